#!/usr/bin/env python3
"""A/B of MXFP4 experts: MXFP8 activations on the scaled MFMA (fp8_mode = 1, gemm_mxa8_kernel) against the weight-only path
(fp8_mode = 0).  Mixtral-8x7B shapes (E=8, K=2, H=4096, I=14336) at M=32 and M=128 (decode), GLM-4.5-Air shapes (E=128, K=8,
H=4096, I=1408) at M=8192 (gpu_prefill), uniform routing, seeded, bf16.  Both engines in one process; each step captured in a
hipGraph, five regions of replays each, alternating the engines; per-kernel times in a separate pass (lkm_set_profiling,
prof_rep); the MXFP8 quantiser is timed on its own -- one captured launch on the token rows and one on an intermediate-sized matrix,
the two launches the mode adds to a step (in the profiled intervals they fall into "sort" and, divided by prof_rep, "GEMM2").  The two
modes compute different things (W4A8 against W4A16), so the outputs are reported, not compared.
On the GPU box:  python tools/mxfp4_a8_ab.py [log]   (default profiles/mxfp4_a8_ab.log)"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from lvllm_amd import _clib, ops  # noqa: E402

HBM, MFMA8 = 8e12, 5e15                                  # bytes / s and fp8-rate flop / s: the ceilings of the fractions
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
        raise SystemExit("mxfp4_a8_ab: no GPU -- this tool measures, it has no CPU path")
    log = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mxfp4_a8_ab.log"
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
                for n, m in (("w4a16", _clib.FP8_W8A16), ("w4a8", _clib.FP8_W8A8))}
        del q13, q2
        say(f"{name} shapes E={E} K={K} H={H} I={I}, MXFP4, bf16; weight bytes w4a16 {engs['w4a16'].engine.weight_bytes()} "
            f"w4a8 {engs['w4a8'].engine.weight_bytes()}")
        for M in Ms:
            x = (torch.randn((M, H), generator=gen, device=dev) / 4).to(torch.bfloat16)
            ids = torch.stack([torch.randperm(E, generator=gen, device=dev)[:K] for _ in range(M)]).to(torch.int32).contiguous()
            tw = torch.softmax(torch.randn((M, K), generator=gen, device=dev), dim=-1).contiguous()
            outs = {n: torch.empty((M, H), dtype=torch.bfloat16 if prefill else torch.float32, device=dev) for n in engs}
            fns = {n: (lambda n=n: outs[n].copy_(engs[n].prefill(x, tw, ids)) if prefill else engs[n].decode(x, tw, ids, out=outs[n])) for n in engs}
            for n in engs:
                fns[n]()
            torch.cuda.synchronize()
            a, b = outs["w4a8"].float().cpu().numpy(), outs["w4a16"].float().cpu().numpy()
            say(f"M={M}: finite {bool(np.isfinite(a).all())}; |w4a8 - w4a16| max {np.abs(a - b).max():.3e} at max |w4a16| {np.abs(b).max():.3e} "
                f"(two different operators)")
            graphs = {n: capture(fns[n]) for n in engs}
            replays = 5 if prefill else 20
            t = {n: [] for n in engs}
            for _ in range(REGIONS):
                for n in engs:
                    t[n].append(region(graphs[n], replays))
            hit = int(torch.unique(ids).numel())
            for n in engs:
                srt, g1, g2, cmb = kernels(engs[n], fns[n])
                roof = (f"GEMM1 weight bytes / time = {hit * 2 * I * H * (0.5 + 1 / 32) / (g1 * 1e-6) / HBM:.3f} of 8 TB/s" if not prefill else
                        f"GEMM1 flop / time = {2.0 * M * K * 2 * I * H / (g1 * 1e-6) / MFMA8:.3f} of 5 PF")
                say(f"M={M} {n:6s} step us {' '.join(f'{v:8.1f}' for v in t[n])} | median {np.median(t[n]):8.1f} spread {max(t[n]) - min(t[n]):6.1f} | "
                    f"sort(+token quantiser) {srt:6.1f} GEMM1 {g1:7.1f} GEMM2(+intermediate quantiser / prof_rep) {g2:7.1f} combine {cmb:6.1f} us | {roof} | "
                    f"{engs[n].engine.last_kernels()['gemm1'][0][:60]} | {engs[n].engine.describe().split('| ', 1)[-1][:100]}")
            act = (torch.randn((M * K, I), generator=gen, device=dev) / 4).to(torch.bfloat16)
            gq = capture(lambda: (ops.quant_mxfp8_rows(x), ops.quant_mxfp8_rows(act)))
            tq = float(np.median([region(gq, replays) for _ in range(REGIONS)]))
            say(f"M={M}: MXFP8 quantiser alone, tokens [{M}, {H}] + intermediate [{M * K}, {I}]: {tq:.1f} us per step = "
                f"{tq / np.median(t['w4a8']):.1%} of the w4a8 step")
            del act, gq
            d = float(np.median(t["w4a16"]) - np.median(t["w4a8"]))
            sp = max(max(t[n]) - min(t[n]) for n in engs)
            say(f"M={M}: w4a8 is {d:+.1f} us ({d / np.median(t['w4a16']):+.1%}) {'faster' if d > 0 else 'SLOWER'} than w4a16 (spread of identical regions {sp:.1f} us)")
        for e in engs.values():
            e.engine.close()
        del engs
        torch.cuda.empty_cache()
    log.parent.mkdir(parents=True, exist_ok=True)
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
