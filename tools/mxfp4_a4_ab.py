#!/usr/bin/env python3
"""A/B of the three MXFP4 engines: weight-only (fp8_mode = 0), MXFP8 activations (fp8_mode = 1, gemm_mxa8_kernel) and MXFP4
activations (fp8_mode = 4, gemm_mxa4_kernel: both operands of the scaled MFMA fp4).  Mixtral-8x7B shapes (E=8, K=2, H=4096, I=14336) at
M=32 and M=128 (decode), GLM-4.5-Air shapes (E=128, K=8, H=4096, I=1408) at M=8192 (gpu_prefill), uniform routing, seeded, bf16.  The
three engines in one process; each step captured in a hipGraph, five regions of replays each, alternating the engines; per-kernel
times in a separate pass (lkm_set_profiling, prof_rep); the MXFP8 and the MXFP4 quantiser pairs are timed on their own -- one captured
launch on the token rows and one on an intermediate-sized matrix, the two launches an activation mode adds to a step (in the profiled
intervals they fall into "sort" and, divided by prof_rep, "GEMM2").  The modes compute different things, so the outputs are reported,
not compared.  The roof of the prefill fraction is the instruction's rate for the mode's operands: 5 PF with an 8-bit or 16-bit token
operand, 10 PF with both operands fp4 (the part's specification).
On the GPU box:  python tools/mxfp4_a4_ab.py [log]   (default profiles/mxfp4_a4_ab.log)"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from lvllm_amd import _clib, ops  # noqa: E402

HBM, ROOF = 8e12, {"w4a16": 5e15, "w4a8": 5e15, "w4a4": 10e15}      # bytes / s and flop / s: the ceilings of the fractions
MODES = (("w4a16", _clib.FP8_W8A16), ("w4a8", _clib.FP8_W8A8), ("w4a4", _clib.FP8_MXA4))
REGIONS, PROF_REP = 5, 8
WORKLOADS = [("Mixtral-8x7B", 8, 2, 4096, 14336, (32, 128), False), ("GLM-4.5-Air", 128, 8, 4096, 1408, (8192,), True)]


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    return g


def region(g, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / replays * 1e3


def kernels(eng, fn):
    eng.engine.set_profiling(True)
    eng.engine.set_tuning(prof_rep=PROF_REP)
    fn()
    torch.cuda.synchronize()
    rows = []
    for _ in range(5):
        fn()
        torch.cuda.synchronize()
        p = eng.engine.get_profile()
        rows.append([p[k] * 1e3 for k in ("sort", "gemm1", "gemm2", "combine")])
    eng.engine.set_tuning(prof_rep=0)
    eng.engine.set_profiling(False)
    return np.median(np.array(rows), axis=0)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_a4_ab: no GPU -- this tool measures, it has no CPU path")
    log = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mxfp4_a4_ab.log"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    for name, E, K, H, I, Ms, prefill in WORKLOADS:
        q13 = torch.randint(0, 256, (E, 2 * I, H // 2), generator=gen, device=dev, dtype=torch.uint8)
        q2 = torch.randint(0, 256, (E, H, I // 2), generator=gen, device=dev, dtype=torch.uint8)
        s13 = torch.randint(118, 123, (E, 2 * I, H // 32), generator=gen, device=dev, dtype=torch.uint8)
        s2 = torch.randint(118, 123, (E, H, I // 32), generator=gen, device=dev, dtype=torch.uint8)
        engs = {n: ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="mxfp4", w13_scale=s13, w2_scale=s2, group_n=1,
                                           group_k=32, fp8_mode=m, max_batch_size=max(Ms), group_max_len=max(Ms))
                for n, m in MODES}
        del q13, q2
        say(f"{name} shapes E={E} K={K} H={H} I={I}, MXFP4, bf16; weight bytes " + " ".join(f"{n} {e.engine.weight_bytes()}" for n, e in engs.items()))
        for M in Ms:
            x = (torch.randn((M, H), generator=gen, device=dev) / 4).to(torch.bfloat16)
            ids = torch.stack([torch.randperm(E, generator=gen, device=dev)[:K] for _ in range(M)]).to(torch.int32).contiguous()
            tw = torch.softmax(torch.randn((M, K), generator=gen, device=dev), dim=-1).contiguous()
            outs = {n: torch.empty((M, H), dtype=torch.bfloat16 if prefill else torch.float32, device=dev) for n in engs}
            fns = {n: (lambda n=n: outs[n].copy_(engs[n].prefill(x, tw, ids)) if prefill else engs[n].decode(x, tw, ids, out=outs[n])) for n in engs}
            for n in engs:
                fns[n]()
            torch.cuda.synchronize()
            o = {n: outs[n].float().cpu().numpy() for n in engs}
            say(f"M={M}: finite {all(bool(np.isfinite(v).all()) for v in o.values())}; |w4a8 - w4a16| max {np.abs(o['w4a8'] - o['w4a16']).max():.3e} "
                f"|w4a4 - w4a16| max {np.abs(o['w4a4'] - o['w4a16']).max():.3e} at max |w4a16| {np.abs(o['w4a16']).max():.3e} (different operators)")
            graphs = {n: capture(fns[n]) for n in engs}
            replays = 5 if prefill else 20
            t = {n: [] for n in engs}
            for _ in range(REGIONS):
                for n in engs:
                    t[n].append(region(graphs[n], replays))
            hit = int(torch.unique(ids).numel())
            gemms = {}
            for n in engs:
                srt, g1, g2, cmb = gemms[n] = kernels(engs[n], fns[n])
                roof = (f"GEMM1 weight bytes / time = {hit * 2 * I * H * (0.5 + 1 / 32) / (g1 * 1e-6) / HBM:.3f} of 8 TB/s" if not prefill else
                        f"GEMM1 flop / time = {2.0 * M * K * 2 * I * H / (g1 * 1e-6) / ROOF[n]:.3f} of {ROOF[n] / 1e15:.0f} PF")
                say(f"M={M} {n:6s} step us {' '.join(f'{v:8.1f}' for v in t[n])} | median {np.median(t[n]):8.1f} spread {max(t[n]) - min(t[n]):6.1f} | "
                    f"sort(+token quantiser) {srt:6.1f} GEMM1 {g1:7.1f} GEMM2(+intermediate quantiser / prof_rep) {g2:7.1f} combine {cmb:6.1f} us | {roof} | "
                    f"{engs[n].engine.last_kernels()['gemm1'][0][:60]} | {engs[n].engine.describe().split('| ', 1)[-1][:100]}")
            act = (torch.randn((M * K, I), generator=gen, device=dev) / 4).to(torch.bfloat16)
            for n, quant in (("w4a8", ops.quant_mxfp8_rows), ("w4a4", ops.quant_mxfp4_rows)):
                gq = capture(lambda: (quant(x), quant(act)))
                tq = float(np.median([region(gq, replays) for _ in range(REGIONS)]))
                say(f"M={M}: {quant.__name__} alone, tokens [{M}, {H}] + intermediate [{M * K}, {I}]: {tq:.1f} us per step = "
                    f"{tq / np.median(t[n]):.1%} of the {n} step")
                del gq
            del act
            sp = max(max(t[n]) - min(t[n]) for n in engs)
            for other in ("w4a16", "w4a8"):
                d = float(np.median(t[other]) - np.median(t["w4a4"]))
                say(f"M={M}: w4a4 is {d:+.1f} us ({d / np.median(t[other]):+.1%}) {'faster' if d > 0 else 'SLOWER'} than {other} (spread of identical regions {sp:.1f} us); "
                    f"GEMM1 {gemms[other][1] - gemms['w4a4'][1]:+.1f} us, GEMM2 {gemms[other][2] - gemms['w4a4'][2]:+.1f} us")
        for e in engs.values():
            e.engine.close()
        del engs
        torch.cuda.empty_cache()
    log.parent.mkdir(parents=True, exist_ok=True)
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
