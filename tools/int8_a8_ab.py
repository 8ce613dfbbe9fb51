#!/usr/bin/env python3
"""A/B of 8-bit experts: int8 weights x per-token int8 activations on the integer MFMA (LKM_W_INT8 with fp8_mode = 1,
gemm_i8a8_kernel) against weight-only int8 (fp8_mode = 0, the same weights as uint8b128) and against block-fp8 W8A8.
Mixtral-8x7B shapes (E=8, K=2, H=4096, I=14336) at M=32 and M=128 (decode), GLM-4.5-Air shapes (E=128, K=8, H=4096, I=1408) at
M=8192 (gpu_prefill), uniform routing, seeded, bf16.  The three engines live in one process; each step is captured in a hipGraph,
five regions of replays each, alternating the engines; per-kernel times come from a separate pass (lkm_set_profiling, prof_rep);
the int8 quantiser is timed on its own -- one captured launch on the token rows and one on an intermediate-sized matrix, the two
launches the mode adds to a step (in the profiled intervals they fall into "sort" and, divided by prof_rep, "GEMM2").  The three
modes are different operators, so the outputs are reported, not compared.
On the GPU box:  python tools/int8_a8_ab.py [log]   (default profiles/int8_a8_ab.log)"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from lvllm_amd import _clib, ops  # noqa: E402

HBM, MFMA8 = 8e12, 5e15                                  # bytes / s and 8-bit-rate op / s: the ceilings of the fractions
REGIONS, PROF_REP = 5, 8
WORKLOADS = [("Mixtral-8x7B", 8, 2, 4096, 14336, (32, 128), False), ("GLM-4.5-Air", 128, 8, 4096, 1408, (8192,), True)]
NEW, OLD = "i8a8", ("i8a16", "fp8a8")


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


def make_engines(E, K, H, I, cap, gen, dev):
    """the same integer weights three ways: signed + fp32 row scales, uint8b128 + bf16 scales per 128 k, and (other bytes, same
    count) e4m3fn + fp32 128 x 128 block scales"""
    kw = dict(top_k=K, act_dtype=torch.bfloat16, max_batch_size=cap, group_max_len=cap)
    q13 = torch.randint(-128, 128, (E, 2 * I, H), generator=gen, device=dev, dtype=torch.int8)
    q2 = torch.randint(-128, 128, (E, H, I), generator=gen, device=dev, dtype=torch.int8)
    s13 = torch.rand((E, 2 * I), generator=gen, device=dev) * 1e-2
    s2 = torch.rand((E, H), generator=gen, device=dev) * 1e-2
    engs = {NEW: ops.RoutedExpertsEngine(q13, q2, fmt="int8", w13_scale=s13, w2_scale=s2, group_n=1, group_k=max(H, I),
                                         fp8_mode=_clib.FP8_W8A8, **kw)}
    u13, u2 = (q13.to(torch.int16) + 128).to(torch.uint8), (q2.to(torch.int16) + 128).to(torch.uint8)
    engs["i8a16"] = ops.RoutedExpertsEngine(u13, u2, fmt="int8", w13_scale=s13.to(torch.bfloat16)[..., None].repeat(1, 1, H // 128),
                                            w2_scale=s2.to(torch.bfloat16)[..., None].repeat(1, 1, I // 128), group_n=1, group_k=128,
                                            fp8_mode=_clib.FP8_W8A16, **kw)
    for u in (u13, u2):
        u[(u & 0x7f) == 0x7f] = 0                        # no NaN bytes
    b13 = torch.rand((E, 2 * I // 128, H // 128), generator=gen, device=dev) * 1e-3
    b2 = torch.rand((E, H // 128, I // 128), generator=gen, device=dev) * 1e-3
    engs["fp8a8"] = ops.RoutedExpertsEngine(u13, u2, fmt="fp8", w13_scale=b13, w2_scale=b2, group_n=128, group_k=128,
                                            fp8_mode=_clib.FP8_W8A8, **kw)
    return engs


def main():
    if not torch.cuda.is_available():
        raise SystemExit("int8_a8_ab: no GPU -- this tool measures, it has no CPU path")
    log = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "int8_a8_ab.log"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    for name, E, K, H, I, Ms, prefill in WORKLOADS:
        engs = make_engines(E, K, H, I, max(Ms), gen, dev)
        torch.cuda.empty_cache()
        say(f"{name} shapes E={E} K={K} H={H} I={I}, 8-bit experts, bf16; weight bytes " + " ".join(f"{n} {e.engine.weight_bytes()}" for n, e in engs.items()))
        for M in Ms:
            x = (torch.randn((M, H), generator=gen, device=dev) / 4).to(torch.bfloat16)
            ids = torch.stack([torch.randperm(E, generator=gen, device=dev)[:K] for _ in range(M)]).to(torch.int32).contiguous()
            tw = torch.softmax(torch.randn((M, K), generator=gen, device=dev), dim=-1).contiguous()
            outs = {n: torch.empty((M, H), dtype=torch.bfloat16 if prefill else torch.float32, device=dev) for n in engs}
            fns = {n: (lambda n=n: outs[n].copy_(engs[n].prefill(x, tw, ids)) if prefill else engs[n].decode(x, tw, ids, out=outs[n])) for n in engs}
            for n in engs:
                fns[n]()
            torch.cuda.synchronize()
            a, b = outs[NEW].float().cpu().numpy(), outs["i8a16"].float().cpu().numpy()
            say(f"M={M}: finite {all(bool(torch.isfinite(o).all()) for o in outs.values())}; |i8a8 - i8a16| max {np.abs(a - b).max():.3e} at max |i8a16| "
                f"{np.abs(b).max():.3e} (two different operators on the same weights)")
            graphs = {n: capture(fns[n]) for n in engs}
            replays = 5 if prefill else 20
            t = {n: [] for n in engs}
            for _ in range(REGIONS):
                for n in engs:
                    t[n].append(region(graphs[n], replays))
            hit = int(torch.unique(ids).numel())
            for n in engs:
                srt, g1, g2, cmb = kernels(engs[n], fns[n])
                roof = (f"GEMM1 weight bytes / time = {hit * 2 * I * H / (g1 * 1e-6) / HBM:.3f} of 8 TB/s" if not prefill else
                        f"GEMM1 op / time = {2.0 * M * K * 2 * I * H / (g1 * 1e-6) / MFMA8:.3f} of 5 P, GEMM2 {2.0 * M * K * I * H / (g2 * 1e-6) / MFMA8:.3f}")
                say(f"M={M} {n:6s} step us {' '.join(f'{v:8.1f}' for v in t[n])} | median {np.median(t[n]):8.1f} spread {max(t[n]) - min(t[n]):6.1f} | "
                    f"sort(+token quantiser) {srt:6.1f} GEMM1 {g1:7.1f} GEMM2(+intermediate quantiser / prof_rep) {g2:7.1f} combine {cmb:6.1f} us | {roof} | "
                    f"{engs[n].engine.last_kernels()['gemm1'][0][:60]} | {engs[n].engine.describe().split('| ', 1)[-1][:100]}")
            act = (torch.randn((M * K, I), generator=gen, device=dev) / 4).to(torch.bfloat16)
            gq = capture(lambda: (ops.quant_int8_rows(x), ops.quant_int8_rows(act)))
            tq = float(np.median([region(gq, replays) for _ in range(REGIONS)]))
            say(f"M={M}: int8 quantiser alone, tokens [{M}, {H}] + intermediate [{M * K}, {I}]: {tq:.1f} us per step = "
                f"{tq / np.median(t[NEW]):.1%} of the i8a8 step")
            del act, gq
            sp = max(max(t[n]) - min(t[n]) for n in engs)
            for o in OLD:
                d = float(np.median(t[o]) - np.median(t[NEW]))
                say(f"M={M}: i8a8 is {d:+.1f} us ({d / np.median(t[o]):+.1%}) {'faster' if d > 0 else 'SLOWER'} than {o} (largest spread of identical regions {sp:.1f} us)")
        for e in engs.values():
            e.engine.close()
        del engs
        torch.cuda.empty_cache()
    log.parent.mkdir(parents=True, exist_ok=True)
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
