"""bench.py's plain run and --dump-outputs: a plain run times one region and nothing else unless --full is given; the outputs of the
last timed step are written as float32 / float64 arrays, large ones as a fixed sample, at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_defaults_and_full():
    a = bench.parse_args([])
    assert not a.full and a.repeats == 1 and a.dump_outputs is None
    a = bench.parse_args(['--full'])
    assert a.full and a.repeats == 3
    assert bench.parse_args(['--repeats', '2']).repeats == 2


def test_output_arrays(monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    conf = torch.rand(2, 40, 40)
    out = {'image0': torch.zeros(2, 1, 8, 8), 'image1': torch.zeros(2, 1, 8, 8), '_static': {}, '_geo_dev': torch.zeros(3),
           'conf_matrix': conf, 'b_ids': torch.tensor([0, 1, 1]), 'mkpts0_f': torch.rand(3, 2).half(), 'mask': torch.tensor([True, False]),
           'w': torch.rand(4, dtype=torch.float64), 'bs': torch.tensor(2), 'note': 'not an array'}
    a = bench.output_arrays(out)
    assert sorted(a) == ['b_ids', 'bs', 'conf_matrix', 'mask', 'mkpts0_f', 'w']
    assert a['conf_matrix'].dtype == np.float32 and a['conf_matrix'].shape == (1000,)
    assert a['b_ids'].dtype == np.float64 and a['b_ids'].tolist() == [0, 1, 1]
    assert a['mkpts0_f'].dtype == np.float32 and a['mkpts0_f'].shape == (3, 2)
    assert a['mask'].tolist() == [1.0, 0.0] and a['w'].dtype == np.float64
    b = bench.output_arrays(out)                          # the same sample in every call
    assert np.array_equal(a['conf_matrix'], b['conf_matrix'])
    assert set(a['conf_matrix'].tolist()) <= set(conf.reshape(-1).tolist())
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 1000)
    with pytest.raises(SystemExit):
        bench.output_arrays(out)


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step(tmp_path):
    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--batch', '2',
                        '--size', '320', '--dump-outputs', str(tmp_path / 'out')], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == steps and line['ms_per_step'] > 0 and line['repeats']['n'] == 1
    assert line['value'] == pytest.approx(2 * steps / (line['ms_per_step'] * steps * 1e-3), rel=1e-6)
    assert not {'roofline', 'side_measurements', 'cpu_baseline'} & set(line)
    files = sorted(os.listdir(tmp_path / 'out'))
    assert {'b_ids.npy', 'mkpts0_f.npy', 'mkpts1_f.npy', 'mconf.npy', 'conf_matrix.npy'} <= set(files)
    arrays = {f: np.load(tmp_path / 'out' / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert len(arrays['b_ids.npy']) == len(arrays['mkpts0_f.npy']) > 0
