#!/usr/bin/env python3
"""A/B of weight-only 8-bit experts: the native one-byte format (fmt "int8", LKM_W_INT8) against the path it replaces, the
16-bit engine on lkm_wna16_expand's output.  Mixtral-8x7B shapes (E=8, H=4096, I=14336, K=2), g128, uint8b128, bf16, uniform
routing, seeded; decode at M=32 and M=128.  Both engines in one process: outputs compared at the decode tolerance, each step
captured in a hipGraph, five regions of 20 replays each, alternating the engines; per-kernel times in a separate pass
(lkm_set_profiling, prof_rep).  On the GPU box:  python tools/int8_native_ab.py [log]   (default profiles/int8_native_ab.log)"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from lvllm_amd import ops  # noqa: E402

E, H, I, K, G = 8, 4096, 14336, 2, 128
HBM = 8e12                                              # bytes / s, the ceiling the fractions are reported against
REGIONS, REPLAYS, PROF_REP = 5, 20, 8


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(5):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    return g


def region(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPLAYS * 1e3


def kernels(eng, fn):
    eng.engine.set_profiling(True)
    eng.engine.set_tuning(prof_rep=PROF_REP)
    fn()
    torch.cuda.synchronize()
    g1, g2 = [], []
    for _ in range(5):
        fn()
        torch.cuda.synchronize()
        p = eng.engine.get_profile()
        g1.append(p["gemm1"] * 1e3)
        g2.append(p["gemm2"] * 1e3)
    eng.engine.set_tuning(prof_rep=0)
    eng.engine.set_profiling(False)
    return float(np.median(g1)), float(np.median(g2))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("int8_native_ab: no GPU -- this tool measures, it has no CPU path")
    log = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "int8_native_ab.log"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    q13 = torch.randint(0, 256, (E, 2 * I, H), generator=gen, device=dev, dtype=torch.uint8)
    q2 = torch.randint(0, 256, (E, H, I), generator=gen, device=dev, dtype=torch.uint8)
    s13 = (torch.rand((E, 2 * I, H // G), generator=gen, device=dev) * 3.5e-3 + 5e-4).to(torch.bfloat16)
    s2 = (torch.rand((E, H, I // G), generator=gen, device=dev) * 3.5e-3 + 5e-4).to(torch.bfloat16)
    native = ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="int8", w13_scale=s13, w2_scale=s2,
                                     group_n=1, group_k=G)
    w13 = ops.wna16_expand(q13, s13, None, 8, G)
    w2 = ops.wna16_expand(q2, s2, None, 8, G)
    expanded = ops.RoutedExpertsEngine(w13, w2, top_k=K, act_dtype=torch.bfloat16, fmt="bf16")
    del w13, w2
    say(f"Mixtral-8x7B shapes E={E} H={H} I={I} K={K}, uint8b128 g{G}, bf16; weight bytes native {native.engine.weight_bytes()} "
        f"expanded {expanded.engine.weight_bytes()}")
    for M in (32, 128):
        x = (torch.randn((M, H), generator=gen, device=dev) / 10).to(torch.bfloat16)
        ids = torch.stack([torch.randperm(E, generator=gen, device=dev)[:K] for _ in range(M)]).to(torch.int32).contiguous()
        tw = torch.softmax(torch.randn((M, K), generator=gen, device=dev), dim=-1).contiguous()
        outs = {n: torch.empty((M, H), dtype=torch.float32, device=dev) for n in ("native", "expanded")}
        engs = {"native": native, "expanded": expanded}
        fns = {n: (lambda n=n: engs[n].decode(x, tw, ids, out=outs[n])) for n in engs}
        for n in engs:
            fns[n]()
        torch.cuda.synchronize()
        a, b = outs["native"].cpu().numpy(), outs["expanded"].cpu().numpy()
        scale = float(np.abs(b).max())
        err = float(np.abs(a - b).max())
        ok = bool(np.isfinite(a).all() and np.allclose(a, b, atol=2e-3 * scale, rtol=1e-2))
        say(f"M={M}: outputs native vs expanded: max |diff| {err:.3e} at max |ref| {scale:.3e} -> {'within' if ok else 'OUTSIDE'} "
            f"atol 2e-3 max|ref|, rtol 1e-2")
        graphs = {n: capture(fns[n]) for n in engs}
        t = {n: [] for n in engs}
        for _ in range(REGIONS):
            for n in engs:
                t[n].append(region(graphs[n]))
        hit = int(torch.unique(ids).numel())
        for n in engs:
            g1, g2 = kernels(engs[n], fns[n])
            bpw = 1.0 + 4.0 / G if n == "native" else 2.0                       # algorithmic bytes per weight (scale pairs included)
            b1 = hit * 2 * I * H * bpw
            say(f"M={M} {n:8s} step us {' '.join(f'{v:7.1f}' for v in t[n])} | median {np.median(t[n]):7.1f} spread {max(t[n]) - min(t[n]):5.1f} "
                f"| GEMM1 {g1:6.1f} us GEMM2 {g2:6.1f} us | GEMM1 weight bytes / time = {b1 / (g1 * 1e-6) / HBM:.3f} of 8 TB/s | "
                f"{engs[n].engine.describe().split('| ', 1)[-1][:110]}")
        d = float(np.median(t["expanded"]) - np.median(t["native"]))
        sp = max(max(t[n]) - min(t[n]) for n in engs)
        say(f"M={M}: native is {d:+.1f} us {'faster' if d > 0 else 'SLOWER'} than expanded (spread of identical regions {sp:.1f} us) -> "
            f"{'ACCEPT' if d > sp else 'NOT accepted'}")
    log.parent.mkdir(parents=True, exist_ok=True)
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
