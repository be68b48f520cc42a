"""Per-workgroup phase timeline of K1's pass A, k1_stats_panel (needs a -DK1_TRACE=1 build:
HIPCC_EXTRA=-DK1_TRACE=1 python -m geoformer_amd.build).  Stamps of each workgroup's SECOND unit: 0 unit start, then per tile t
1+6t top of the tile, 2+6t tile landed (wait + barrier), 3+6t MFMAs done, 4+6t maxima / rescale, 5+6t exponentials and sums."""
import sys, ctypes
import numpy as np, torch
sys.path.insert(0, '.')
from geoformer_amd import ops, _lib
N, L, S, C = 8, 6400, 6400, 256
f0 = (torch.randn(N, L, C, device='cuda') * 1.3).half()
f1 = (f0[:, torch.randperm(S, device='cuda')].float() + 0.4 * torch.randn(N, S, C, device='cuda')).half()
for _ in range(3):
    ops.dual_softmax_match(f0, f1, 0.1, 0.0, (80, 80), (80, 80), 8.0)
torch.cuda.synchronize()
buf = np.zeros(512 * 4 * 32, dtype=np.int64)
ctypes.CDLL(_lib.LIB_PATH).gf_debug_k1_trace(buf.ctypes.data_as(ctypes.c_void_p))
t = buf.reshape(512, 4, 32)[:, 0, :25]
d = t - t[:, :1]
m = np.median(d, axis=0)
print('pass A, second unit of every workgroup, median clocks from unit start (wave 0):')
for tl in range(4):
    b = 1 + 6 * tl
    print(f'tile {tl}: top {int(m[b])} | wait + barrier {int(m[b+1]-m[b])} | DMA issue + MFMAs {int(m[b+2]-m[b+1])} | maxima / rescale {int(m[b+3]-m[b+2])} | exponentials, sums {int(m[b+4]-m[b+3])} | to next top {int(m[b+6]-m[b+4]) if b + 6 < 25 else -1}')
