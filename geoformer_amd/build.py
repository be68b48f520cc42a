"""In-tree build of libgeoformer_hip.so: hipcc --offload-arch=gfx950 over geoformer_amd/csrc/*.hip.

No cmake, no torch headers: the library is a plain C-ABI shared object (include/geoformer_hip.h).
Objects are cached per source under csrc/_obj keyed on content hashes, so rebuilding after an edit
recompiles only what changed.
"""
import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(CSRC, '_obj')
LIB = os.path.join(HERE, 'libgeoformer_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-value'] + os.environ.get('HIPCC_EXTRA', '').split()
# the host C++ compiler; where none is on PATH, the clang that hipcc itself drives (same flags, no offload)
HOST_CXX = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or '/opt/rocm/lib/llvm/bin/clang++'
HOST_FLAGS = ['-O2', '-ffp-contract=off', '-std=c++17', '-fPIC']
POSE_HOST_LIB = os.path.join(OBJ, 'libpose_host.so')
WARP_HOST_LIB = os.path.join(OBJ, 'libwarp_host.so')
KEYPOINT_HOST_LIB = os.path.join(OBJ, 'libkeypoint_host.so')
FUND_HOST_LIB = os.path.join(OBJ, 'libfund_host.so')
ABSPOSE_HOST_LIB = os.path.join(OBJ, 'libabspose_host.so')
TRI_HOST_LIB = os.path.join(OBJ, 'libtri_host.so')
COVIS_HOST_LIB = os.path.join(OBJ, 'libcovis_host.so')
BA_HOST_LIB = os.path.join(OBJ, 'libba_host.so')
CAMERA_HOST_LIB = os.path.join(OBJ, 'libcamera_host.so')
RELPOSE_HOST_LIB = os.path.join(OBJ, 'librelpose_host.so')


def _headers_digest():
    h = hashlib.sha256()
    for d in (CSRC, os.path.join(os.path.dirname(HERE), 'include')):
        for f in sorted(os.listdir(d)):
            if f.endswith('.h'):
                h.update(open(os.path.join(d, f), 'rb').read())
    h.update(' '.join(FLAGS).encode())
    return h.hexdigest()


def _file_flags(body):
    """Per-file compiler flags: a `// hipcc-flags: ...` line among the first lines of the source."""
    for line in body.split(b'\n')[:5]:
        if line.startswith(b'// hipcc-flags:'):
            return line[len(b'// hipcc-flags:'):].decode().split()
    return []


def _compile(src, hdig, verbose):
    body = open(src, 'rb').read()
    extra = _file_flags(body)
    tag = hashlib.sha256(body + hdig.encode()).hexdigest()[:16]
    obj = os.path.join(OBJ, os.path.basename(src) + '.' + tag + '.o')
    if not os.path.exists(obj):
        for old in os.listdir(OBJ):
            if old.startswith(os.path.basename(src) + '.'):
                os.remove(os.path.join(OBJ, old))
        cmd = [HIPCC, *FLAGS, *extra, '-c', src, '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return obj


def _build_host_lib(lib, stamp_name, src, headers, verbose):
    os.makedirs(OBJ, exist_ok=True)
    h = hashlib.sha256()
    for f in (src, *headers):
        h.update(open(f, 'rb').read())
    h.update(' '.join([HOST_CXX, *HOST_FLAGS]).encode())
    stamp_file = os.path.join(OBJ, stamp_name)
    if not (os.path.exists(lib) and os.path.exists(stamp_file) and open(stamp_file).read() == h.hexdigest()):
        cmd = [HOST_CXX, *HOST_FLAGS, '-shared', '-o', lib, src]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        open(stamp_file, 'w').write(h.hexdigest())
    return lib


def build_pose_host(verbose=True):
    """TEST INFRASTRUCTURE: the serial host form of the essential-matrix RANSAC (csrc/host/pose_host.cpp over csrc/pose_solver.h, the
    text k_pose.hip compiles for the device), built by the host C++ compiler without offload.  Only tests load it."""
    return _build_host_lib(POSE_HOST_LIB, 'pose_host.stamp', os.path.join(CSRC, 'host', 'pose_host.cpp'),
                           (os.path.join(CSRC, 'pose_solver.h'), os.path.join(CSRC, 'solver_common.h'), os.path.join(CSRC, 'gf_hash.h')), verbose)


def build_warp_host(verbose=True):
    """TEST INFRASTRUCTURE: the perspective warp and the brightness / contrast rule of the homography-pair generator on the host
    (csrc/host/warp_host.cpp over csrc/warp_spec.h, the text k_homo_pair.hip compiles for the device).  Only tests load it."""
    return _build_host_lib(WARP_HOST_LIB, 'warp_host.stamp', os.path.join(CSRC, 'host', 'warp_host.cpp'),
                           (os.path.join(CSRC, 'warp_spec.h'),), verbose)


def build_keypoint_host(verbose=True):
    """TEST INFRASTRUCTURE and CPU reference: the keypoint consolidation for SfM, serially on the host (csrc/host/keypoint_host.cpp over
    csrc/keypoint_spec.h, the text k_keypoints.hip compiles for the device).  Only tests and tools/keypoint_probe.py load it."""
    return _build_host_lib(KEYPOINT_HOST_LIB, 'keypoint_host.stamp', os.path.join(CSRC, 'host', 'keypoint_host.cpp'),
                           (os.path.join(CSRC, 'keypoint_spec.h'),), verbose)


def build_fund_host(verbose=True):
    """TEST INFRASTRUCTURE: the serial host form of the fundamental-matrix RANSAC (csrc/host/fund_host.cpp over csrc/fund_solver.h, the
    text k_fundamental.hip compiles for the device).  Only tests load it."""
    return _build_host_lib(FUND_HOST_LIB, 'fund_host.stamp', os.path.join(CSRC, 'host', 'fund_host.cpp'),
                           tuple(os.path.join(CSRC, h) for h in ('fund_solver.h', 'solver_common.h', 'keypoint_spec.h', 'gf_hash.h')), verbose)


def build_abspose_host(verbose=True):
    """TEST INFRASTRUCTURE: the serial host form of the absolute-pose RANSAC and of the 3-D map lookup (csrc/host/abspose_host.cpp over
    csrc/abs_solver.h, the text k_abspose.hip compiles for the device).  Only tests load it."""
    return _build_host_lib(ABSPOSE_HOST_LIB, 'abspose_host.stamp', os.path.join(CSRC, 'host', 'abspose_host.cpp'),
                           tuple(os.path.join(CSRC, h) for h in ('abs_solver.h', 'fund_solver.h', 'solver_common.h', 'keypoint_spec.h', 'gf_hash.h')),
                           verbose)


def build_tri_host(verbose=True):
    """TEST INFRASTRUCTURE and CPU reference: the serial host form of the track building and the triangulation (csrc/host/tri_host.cpp over
    csrc/tri_solver.h, the text k_triangulate.hip compiles for the device).  Only tests and tools/triangulate_probe.py load it."""
    return _build_host_lib(TRI_HOST_LIB, 'tri_host.stamp', os.path.join(CSRC, 'host', 'tri_host.cpp'),
                           tuple(os.path.join(CSRC, h) for h in ('tri_solver.h', 'abs_solver.h', 'fund_solver.h', 'solver_common.h',
                                                                 'keypoint_spec.h', 'gf_hash.h')), verbose)


def build_covis_host(verbose=True):
    """TEST INFRASTRUCTURE and CPU reference: the serial host form of the covisibility clustering and the 2-D - 3-D rows of sparse
    localisation (csrc/host/covis_host.cpp over csrc/covis_spec.h, the text k_covis.hip compiles for the device).  Only tests and
    tools/covis_probe.py load it."""
    return _build_host_lib(COVIS_HOST_LIB, 'covis_host.stamp', os.path.join(CSRC, 'host', 'covis_host.cpp'),
                           (os.path.join(CSRC, 'covis_spec.h'),), verbose)


def build_ba_host(verbose=True):
    """TEST INFRASTRUCTURE and CPU reference: the serial host form of the bundle adjustment (csrc/host/ba_host.cpp over csrc/ba_spec.h, the
    text k_bundle.hip compiles for the device).  Only tests and tools/bundle_probe.py load it."""
    return _build_host_lib(BA_HOST_LIB, 'ba_host.stamp', os.path.join(CSRC, 'host', 'ba_host.cpp'),
                           tuple(os.path.join(CSRC, h) for h in ('ba_spec.h', 'ba_pcg_spec.h', 'tri_solver.h', 'abs_solver.h', 'fund_solver.h', 'solver_common.h',
                                                                 'keypoint_spec.h', 'gf_hash.h')), verbose)


def build_camera_host(verbose=True):
    """TEST INFRASTRUCTURE and CPU reference: the serial host form of the lens-distortion rule (csrc/host/camera_host.cpp over
    csrc/camera_spec.h, the text k_camera.hip compiles for the device).  Only tests and tools/camera_probe.py load it."""
    return _build_host_lib(CAMERA_HOST_LIB, 'camera_host.stamp', os.path.join(CSRC, 'host', 'camera_host.cpp'),
                           (os.path.join(CSRC, 'camera_spec.h'),), verbose)


def build_relpose_host(verbose=True):
    """TEST INFRASTRUCTURE: the serial host form of the calibrated two-view RANSAC (csrc/host/relpose_host.cpp over csrc/rel_solver.h, the
    text k_relpose.hip compiles for the device).  Only tests load it."""
    return _build_host_lib(RELPOSE_HOST_LIB, 'relpose_host.stamp', os.path.join(CSRC, 'host', 'relpose_host.cpp'),
                           tuple(os.path.join(CSRC, h) for h in ('rel_solver.h', 'pose_solver.h', 'fund_solver.h', 'solver_common.h',
                                                                 'keypoint_spec.h', 'gf_hash.h')), verbose)


def build(verbose=True, jobs=4):
    os.makedirs(OBJ, exist_ok=True)
    build_camera_host(verbose)
    build_pose_host(verbose)
    build_warp_host(verbose)
    build_keypoint_host(verbose)
    build_fund_host(verbose)
    build_abspose_host(verbose)
    build_tri_host(verbose)
    build_covis_host(verbose)
    build_ba_host(verbose)
    build_relpose_host(verbose)
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.hip'))
    hdig = _headers_digest()
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(lambda s: _compile(s, hdig, verbose), srcs))
    stamp = hashlib.sha256(' '.join(objs).encode()).hexdigest()
    stamp_file = os.path.join(OBJ, 'link.stamp')
    if not (os.path.exists(LIB) and os.path.exists(stamp_file) and open(stamp_file).read() == stamp):
        cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB, *objs]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        open(stamp_file, 'w').write(stamp)
    return LIB


if __name__ == '__main__':
    print(build(verbose='-q' not in sys.argv))
