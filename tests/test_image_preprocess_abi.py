"""CPU checks of the image-preprocessing entry point of the C ABI (gf_image_gray_resize): declared in the header, bound with
the same argument count, exported by the built library, and every invalid argument is reported as status -1 with a message
that names the argument - before anything touches a device (this file runs on a machine without one)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'geoformer_hip.h')
NAME = 'gf_image_gray_resize'


@pytest.fixture(scope='module')
def lib():
    from geoformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _header_arguments():
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'^\s*int\s+' + NAME + r'\s*\(([^;]*?)\)\s*;', txt, flags=re.M | re.S)
    assert m, f'{NAME} is not declared in include/geoformer_hip.h'
    return [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]


def test_declared_bound_and_exported(lib):
    args = _header_arguments()
    assert len(args) == 10
    assert NAME in lib.SIGNATURES, f'{NAME} has no ctypes signature'
    res, argtypes = lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[4] is ctypes.c_longlong and 'long long' in args[4]            # the row stride in bytes
    syms = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r' T ' + NAME + r'$', syms, flags=re.M), f'{NAME} is not exported by {lib.LIB_PATH}'
    assert hasattr(lib.lib(), NAME)
    hdr = open(HEADER).read()
    assert lib.lib().gf_abi_version() == lib.ABI_VERSION == int(re.search(r'#define GF_ABI_VERSION (\d+)', hdr).group(1)) == 4
    for const in ('GF_IMAGE_U8', 'GF_IMAGE_F32_NORMALISED', 'GF_IMAGE_F32_NORMALISED_RCP'):
        assert int(re.search(const + r'\s*=\s*(\d+)', hdr).group(1)) == getattr(lib, const)


def test_invalid_arguments_come_back_as_status_codes(lib):
    h = lib.lib()
    U8, F32 = lib.GF_IMAGE_U8, lib.GF_IMAGE_F32_NORMALISED
    buf = ctypes.create_string_buffer(4096)                      # host memory: an accepted call would fault, a rejected one never looks
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(src=p, channels=3, hs=8, ws=8, stride=24, dst=p, kind=U8, ht=4, wt=4)

    def call(**kw):
        a = dict(good, **kw)
        return h.gf_image_gray_resize(a['src'], a['channels'], a['hs'], a['ws'], a['stride'], a['dst'], a['kind'], a['ht'], a['wt'], None)

    cases = [
        (dict(src=None), b'src'),
        (dict(dst=None), b'dst'),
        (dict(channels=0), b'channels'), (dict(channels=2), b'channels'), (dict(channels=4), b'channels'),
        (dict(hs=0), b'hs'), (dict(ws=-1), b'ws'), (dict(ht=0), b'ht'), (dict(wt=-3), b'wt'),
        (dict(stride=23), b'src_row_stride_bytes'), (dict(channels=1, stride=7), b'src_row_stride_bytes'),
        (dict(stride=-24), b'src_row_stride_bytes'),
        (dict(kind=3), b'dst_kind'), (dict(kind=-1), b'dst_kind'), (dict(kind=255), b'dst_kind'),
        (dict(kind=F32, channels=5), b'channels'),
    ]
    for kw, word in cases:
        rc = call(**kw)
        msg = h.gf_last_error()
        assert rc == -1, (kw, rc)
        assert NAME.encode() in msg and word in msg, (kw, msg)
