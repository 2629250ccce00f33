#!/usr/bin/env python3
"""The Q target's tail kernel alone (mms_q_heads_backup, csrc/q_kernels.hip): G = 2 with backup and logp, 10 warm-up calls, then 200
back-to-back calls between two events, at (M, H) = (65536, 1024), (8192, 1024), (65536, 256).  Prints one JSON line: microseconds per
call and TB/s on the bytes the kernel must move, (8 M H + 13 M) -- the 65536 x 256 problem is 134 MB and stays in the Infinity Cache.
`MMS_LIB=<other libmms.so>` times another build of the library (A/B: profiles/q_heads_tail_ab.jsonl).

    python tools/bench_q_tail.py
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _lib.for_device("cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = {"lib": os.path.basename(_lib.LIB_PATH)}
    for M, H in ((65536, 1024), (8192, 1024), (65536, 256)):
        h = [torch.randn(M, H, device="cuda") for _ in range(2)]
        w = [torch.randn(1, H, device="cuda") for _ in range(2)]
        b = [torch.randn(1, device="cuda") for _ in range(2)]
        r, logp = torch.randn(M, device="cuda"), torch.randn(M, device="cuda")
        d = torch.zeros(M, dtype=torch.uint8, device="cuda")
        out = torch.empty(M, device="cuda")

        def call():
            _lib.check(L.mms_q_heads_backup(dev, M, H, p(h[0]), p(w[0]), p(b[0]), None, p(h[1]), p(w[1]), p(b[1]), None, p(r), p(d), p(logp),
                                            0.99, 0.2, p(out), stream), None, "mms_q_heads_backup", L)

        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1000 / 200
        res["%dx%d" % (M, H)] = {"us": round(us, 2), "TBps": round((8 * M * H + 13 * M) / us / 1e6, 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
