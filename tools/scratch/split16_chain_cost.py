#!/usr/bin/env python3
"""Time of the PPO pair's hidden layers on the two-fp16-plane layer kernel as a CHAIN (both networks, 4096 rows, the bench's widths:
388 -> 1024 planes -> 1024 planes -> 512 fp32), beside each launch repeated on its own: a consumer that pays for what its producer's
store policy left behind (lines dropped from the writer's L2, dirty lines at the boundary) shows in the chain and not in the
single-launch loops of split16_fixed_cost.py.  Five rounds of 200 iterations per series; us per iteration, min / median.
MMS_LIB selects the build (one process per build)."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from massive_marl_benchmark_amd import _lib  # noqa: E402

L, d, stream = _lib.for_device(torch.device("cuda"))
M, K1, H, N3, G = 4096, 388, 1024, 512, 2
arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
nb = lambda r, K: r * ((K + 31) // 32) * 128
f32 = lambda n: torch.empty(n, device="cuda")
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
torch.manual_seed(0)


def planes(rows, K, scale):
    src = [torch.randn(rows, K, device="cuda") * scale for _ in range(G)]
    p, s, i = [u8(nb(rows, K)) for _ in range(G)], [f32(rows) for _ in range(G)], [f32(rows) for _ in range(G)]
    assert L.mms_split_planes16_group(d, G, rows, K, 0, arr(src), arr(p), arr(s), arr(i), 0, 0, None, None, None, None, 0.0, stream) == 0
    return p, i, src


xp, xi, _x = planes(M, K1, 1.0)
w1p, w1i, _w1 = planes(H, K1, K1 ** -0.5)
w2p, w2i, _w2 = planes(H, H, H ** -0.5)
w3p, w3i, _w3 = planes(N3, H, H ** -0.5)
b1, b2, b3 = ([torch.zeros(n, device="cuda") for _ in range(G)] for n in (H, H, N3))
# hidden activations are O(1) behind the ELU: a fixed row scale of 64 (split16_fixed_cost.py's) keeps both planes well inside fp16
ysc = [torch.full((M,), 64.0, device="cuda") for _ in range(G)]
yinv = [torch.full((M,), 1.0 / 64.0, device="cuda") for _ in range(G)]
h1, h2 = [u8(nb(M, H)) for _ in range(G)], [u8(nb(M, H)) for _ in range(G)]
y3 = [u8(M * N3 * 4) for _ in range(G)]
a = {k: arr(v) for k, v in dict(xp=xp, xi=xi, w1p=w1p, w1i=w1i, w2p=w2p, w2i=w2i, w3p=w3p, w3i=w3i, b1=b1, b2=b2, b3=b3, ysc=ysc, yinv=yinv,
                                h1=h1, h2=h2, y3=y3).items()}
S = L.mms_linear_group_act_split16
l1 = lambda: S(d, G, M, H, K1, a["xp"], a["w1p"], a["b1"], a["h1"], a["xi"], a["w1i"], a["ysc"], 1, 1, None, None, None, None, None, 0, stream)
l2 = lambda: S(d, G, M, H, H, a["h1"], a["w2p"], a["b2"], a["h2"], a["yinv"], a["w2i"], a["ysc"], 1, 1, None, None, None, None, None, 0, stream)
l3 = lambda: S(d, G, M, N3, H, a["h2"], a["w3p"], a["b3"], a["y3"], a["yinv"], a["w3i"], None, 1, 0, None, None, None, None, None, 0, stream)
series = {"l1": (l1,), "l2": (l2,), "l3": (l3,), "l2_l3": (l2, l3), "l1_l2_l3": (l1, l2, l3)}
for fn in (l1, l2, l3):
    assert fn() == 0, _lib.last_error(None)
torch.cuda.synchronize()
assert bool(torch.isfinite(y3[0].view(torch.float32)).all())
out = {"lib": os.path.basename(os.environ.get("MMS_LIB", "default"))}
for name, fns in series.items():
    for _ in range(20):
        for fn in fns:
            fn()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(200):
            for fn in fns:
                fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 5)
    times.sort()
    out[name + "_us"] = [round(times[0], 2), round(times[2], 2)]
print(json.dumps(out), flush=True)
