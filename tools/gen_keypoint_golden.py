"""Records tests/golden/g19_keypoint_quantize.npz: synthetic float32 pair matches and what the reference's own
`matches_to_keypoint_ids` (eval_tool/immatch/utils/localize_sfm_helper.py) makes of them - keypoint lists per image and id rows per pair.

    python tools/gen_keypoint_golden.py /path/to/reference/checkout [--out tests/golden/g19_keypoint_quantize.npz]

The reference module is imported from the checkout given on the command line; third-party modules it imports at load time and that are
absent here (h5py; tqdm where missing) get inert stand-ins - none of them is touched by the four functions that run.  Runs on the
CPU only.  The archive is written with fixed zip timestamps, so the same inputs give the same bytes.

Inputs: 5 images of 200 x 150 on a quarter-pixel lattice, 8 pairs: one in reversed image order (2, 0), one without rows, one entirely
below the score threshold, one listed twice; scores distinct within each pair (the reference's tie order is undefined).  Image 0
carries a dense cluster inside one 48-pixel cell, so that (psize, dthres) = (48, 0.5) gives a cell more than 64 centres.
Cases: (48, 4), (48, 0.5), (16, 6) with the uniqueness filter on and off, and the exact mode (psize = dthres = -1).
Rows under the filter are stored sorted lexicographically (the reference returns them in a set's order)."""
import argparse
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

SC_THRES = 0.25
CASES = [(48.0, 4.0, 1), (48.0, 4.0, 0), (48.0, 0.5, 1), (48.0, 0.5, 0), (16.0, 6.0, 1), (16.0, 6.0, 0), (-1.0, -1.0, 1)]
PAIRS = [(0, 1), (1, 2), (2, 0), (0, 3), (3, 4), (1, 4), (2, 3), (0, 1)]
ROWS = [260, 240, 250, 230, 0, 60, 220, 200]
W, H = 200, 150


def make_inputs():
    rng = np.random.RandomState(19)
    matches, scores = [], []
    for q, ((i0, i1), n) in enumerate(zip(PAIRS, ROWS)):
        m = np.empty((n, 4), np.float32)
        for s, im in enumerate((i0, i1)):
            x = rng.randint(0, 4 * W, n).astype(np.float32) / np.float32(4)
            y = rng.randint(0, 4 * H, n).astype(np.float32) / np.float32(4)
            if im == 0:                                     # the dense cluster: cell (1, 1) of image 0 at psize 48
                dense = rng.rand(n) < 0.45
                x = np.where(dense, np.float32(48) + rng.randint(0, 4 * 48, n).astype(np.float32) / np.float32(4), x)
                y = np.where(dense, np.float32(48) + rng.randint(0, 4 * 48, n).astype(np.float32) / np.float32(4), y)
            m[:, 2 * s], m[:, 2 * s + 1] = x, y
        if n >= 8:                                          # repeated points and a signed zero for the exact mode
            m[3] = m[1]
            m[5, :2] = m[2, :2]
            m[6, 0], m[7, 0] = np.float32(0.0), np.float32(-0.0)
            m[6, 1] = m[7, 1] = np.float32(7.25)
        sc = (np.float32(0.05) + np.float32(0.9) * rng.permutation(n).astype(np.float32) / np.float32(max(n, 1))).astype(np.float32)
        if q == 5:
            sc = (sc * np.float32(0.2)).astype(np.float32)  # entirely below the threshold
        assert len(np.unique(sc)) == n
        matches.append(m), scores.append(sc)
    offsets = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int32)
    return np.concatenate(matches).astype(np.float32), np.concatenate(scores).astype(np.float32), offsets, np.array(PAIRS, np.int32)


def import_reference(root):
    for name in ('h5py', 'tqdm'):
        if importlib.util.find_spec(name) is None:
            stub = types.ModuleType(name)
            stub.tqdm = lambda it=None, **kw: it
            sys.modules[name] = stub
    # the module file alone, not through its packages (their __init__ files import the matcher and its dependencies)
    path = os.path.join(os.path.abspath(root), 'eval_tool', 'immatch', 'utils', 'localize_sfm_helper.py')
    spec = importlib.util.spec_from_file_location('localize_sfm_helper', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, matches, scores, offsets, pair_images, psize, dthres, unique):
    n_images = int(pair_images.max()) + 1
    all_kp, ids = {}, []
    for q, (i0, i1) in enumerate(pair_images):
        m, s = matches[offsets[q]:offsets[q + 1]], scores[offsets[q]:offsets[q + 1]]
        valid = np.where(s >= SC_THRES)[0]
        r = np.asarray(ref.matches_to_keypoint_ids(m[valid], s[valid], f'im{i0}', f'im{i1}', all_kp, dthres, psize, bool(unique)))
        r = r.reshape(-1, 2).astype(np.int32)
        if unique and psize > 0 and dthres > 0 and len(r):
            r = r[np.lexsort((r[:, 1], r[:, 0]))]
        ids.append(r)
    kps = [np.asarray(all_kp[f'im{i}']['kps'], np.float32).reshape(-1, 2) if f'im{i}' in all_kp else np.zeros((0, 2), np.float32)
           for i in range(n_images)]
    most = max((len(c['means']) for d in all_kp.values() for c in d.get('kp_means', {}).values()), default=0)
    return kps, ids, most


def write_npz(path, arrays):
    """numpy's .npz layout with a fixed timestamp per member: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                                  'g19_keypoint_quantize.npz'))
    args = ap.parse_args()
    ref = import_reference(args.reference)
    matches, scores, offsets, pair_images = make_inputs()
    out = {'matches': matches, 'scores': scores, 'pair_offsets': offsets, 'pair_images': pair_images,
           'sc_thres': np.array(SC_THRES, np.float32), 'cases': np.array(CASES, np.float32)}
    for c, (psize, dthres, unique) in enumerate(CASES):
        kps, ids, most = run_reference(ref, matches, scores, offsets, pair_images, psize, dthres, unique)
        if (psize, dthres) == (48.0, 0.5):
            assert most > 64, most
        out[f'c{c}_keypoints'] = np.concatenate(kps).astype(np.float32)
        out[f'c{c}_kp_offsets'] = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int32)
        out[f'c{c}_ids'] = np.concatenate(ids).astype(np.int32).reshape(-1, 2)
        out[f'c{c}_ids_offsets'] = np.concatenate([[0], np.cumsum([len(r) for r in ids])]).astype(np.int32)
        out[f'c{c}_most_centres'] = np.array(most, np.int32)
        print(f'case {c} (psize {psize}, dthres {dthres}, unique {unique}): {sum(len(k) for k in kps)} keypoints, '
              f'{sum(len(r) for r in ids)} id rows, most centres in a cell {most}')
    write_npz(args.out, out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
