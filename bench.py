#!/usr/bin/env python3
"""bench.py -- MoE-layer decode throughput of the MI355X-native routed-expert path.

Metric (BASELINE.json): MoE-layer decode tokens/s + grouped-GEMM % of roofline, Mixtral-8x7B.
Headline workload: BASELINE.json configs[1] -- Mixtral-8x7B bf16 experts (E=8, top-2, H=4096, I=14336), decode
batch 32 per GPU, synthetic hidden states / router logits / random-init weights, all resident in HBM before
the timed region.  One "step" = one pass of the hot path over the batch:
router top-k (a1) -> scatter (sort) -> grouped GEMM1 + SiLU-mul -> grouped GEMM2 -> top-k combine.

`python bench.py --gpus N` works by itself: without WORLD_SIZE in the environment it re-launches itself as N ranks
under torch.distributed.run (one rank per GPU, RCCL); launched BY torch.distributed.run it simply is one of the
ranks.  N>1: experts are sharded E/N per rank (linear placement), every rank keeps its own 32-token batch, each
token visits the ranks that own its experts through ONE all-to-all out and ONE back (lvllm_amd/ep.py) -- weak
scaling; value = all ranks' tokens / max-over-ranks time.  The whole expert-parallel step is captured in a
hipGraph like the single-GPU step.

A plain run (`--gpus N --steps K --warmup W`) does what the headline figure needs and no more: it sets up, warms up, times
the K steps, writes the arrays of the last timed step if `--dump-outputs DIR` is given, and prints the headline line with
`roofline` and `cpu_baseline` null.  Whatever below takes runs of its own -- `roofline`, `long_run`, `cpu_baseline`, the extra
workloads, the `--full-out` side file -- is behind `--full`.

Output (rank 0, stdout).  The LAST line is the headline object and nothing else (contract in the task statement:
metric, value, ms_per_step, steps, dtype, config.workload, `roofline` of the dominant kernel = GEMM1 -- algorithmic
weight bytes / the median of its HIP-event durations on the launch stream, kernel name taken from the launch --
and `cpu_baseline`: at N=1 the reference's own in-tree CPU kernel via oracle/_ref, with the CPU oracle port beside
it), kept under 4 KB so that it survives any tail the driver keeps (round 4's 22 KB line did not).  BEFORE it, one
short JSON line per extra workload (`{"extra_workload": ...}`): the other BASELINE configurations timed the same way in
the same run -- at N=1 Mixtral fp8-W8A8 M=32 (the north-star fp8 number), Mixtral int4-g128 M=128 (configs[2]), the
GLM-4.5-Air prefill shapes (configs[4]); at every N that divides 256 the full configs[3] workload (DeepSeek-V3 style:
256 fp8 experts, grouped sigmoid+bias top-8 of 4/8 groups, global decode batch 256, EP=N all-to-all).  The complete
records (every field of round 4's line) go to the side file `--full-out` (default gpurun_out/bench_full.json).
The engine runs with its DEFAULT settings (first-call autotune off, as lk_moe / modular users get it); `--autotune`
turns the plan search on and says so in config.autotune.
"""
from __future__ import annotations

import argparse
import gc
import json
import math
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

# cpu_baseline: the reference kernel (oracle/_ref) runs on LLVM's OpenMP runtime, torch and the port on GNU's.  Its team is
# pinned core by core (the reference pins its lk_moe pool with LK_THREAD_BINDING, numa_utils.py:508-527) through the
# LLVM-only KMP_AFFINITY: the portable OMP_PROC_BIND / OMP_PLACES would also bind torch's libgomp, whose initialisation
# then confines the main thread to ONE core -- and libomp, loaded later, inherits that two-CPU mask for its whole team
# (measured: 170-185 ms per step at every team size instead of 10-25 ms; profiles/r04_cpu_baseline_binding.log).
os.environ.setdefault("KMP_AFFINITY", "granularity=core,compact")

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

_GLM_ROUTER = dict(kind="grouped", n_group=1, topk_group=1, scoring="sigmoid", routed_scaling=1.0, bias=True)
WORKLOADS = {
    # name: E experts, K top-k, H hidden, I intermediate, M tokens per GPU, weight format
    "mixtral8x7b_bf16_decode_m32": dict(E=8, K=2, H=4096, I=14336, M=32, fmt="bf16"),
    "mixtral8x7b_int4g128_decode_m128": dict(E=8, K=2, H=4096, I=14336, M=128, fmt="int4", g=128),
    # MOE_WNA16.gpu_prefill (routed_experts.py:1884-1899): the same experts at a prefill chunk of 4096 tokens (MFMA-bound)
    "mixtral8x7b_int4g128_prefill_m4096": dict(E=8, K=2, H=4096, I=14336, M=4096, fmt="int4", g=128, prefill=True),
    # the same checkpoint in the engine's opt-in fast int4 mode (LkmConfig.int4_mode: group scale on fp32 partial sums)
    "mixtral8x7b_int4g128_fast_decode_m128": dict(E=8, K=2, H=4096, I=14336, M=128, fmt="int4", g=128, int4_mode=1),
    # ... and with ZERO POINTS (AWQ-style asymmetric uint4; LkmConfig.int4_mode = LKM_INT4_ZP: T((q - zp) s) decoded in registers
    # from the packed image).  The synthetic zero points are all 8, so the layer is the symmetric one above, number for number.
    "mixtral8x7b_int4g128_zp_decode_m128": dict(E=8, K=2, H=4096, I=14336, M=128, fmt="int4", g=128, int4_mode=2),
    "qwen3_30b_a3b_bf16_decode_m1": dict(E=128, K=8, H=2048, I=768, M=1, fmt="bf16"),
    # BASELINE.json configs[3]: DeepSeek-V3-style layer -- 256 fp8 (128x128 block) experts, group-limited sigmoid
    # router with score-correction bias, GLOBAL decode batch 256 split over the ranks (M_global), experts sharded
    # 256/N per rank.  N=1 holds all 256 experts (11.3 GB of fp8) on one GPU.
    "dsv3_fp8w8a8_ep_decode_b256": dict(E=256, K=8, H=7168, I=2048, M_global=256, fmt="fp8", fp8_mode=1,
                                        router=dict(kind="grouped", n_group=8, topk_group=4, scoring="sigmoid",
                                                    routed_scaling=2.5, bias=True)),
    "dsv3_fp8w8a16_ep_decode_b256": dict(E=256, K=8, H=7168, I=2048, M_global=256, fmt="fp8", fp8_mode=0,
                                         router=dict(kind="grouped", n_group=8, topk_group=4, scoring="sigmoid",
                                                     routed_scaling=2.5, bias=True)),
    # per-rank slice of configs[3] with pre-dispatched rows (round-1 workload, kept for tools/report.py)
    "dsv3_ep8_rank_bf16_rows256": dict(E=32, K=1, H=7168, I=2048, M=256, fmt="bf16"),
    "dsv3_ep8_rank_fp8w8a8_rows256": dict(E=32, K=1, H=7168, I=2048, M=256, fmt="fp8", fp8_mode=1),
    "dsv3_ep8_rank_fp8w8a16_rows256": dict(E=32, K=1, H=7168, I=2048, M=256, fmt="fp8", fp8_mode=0),
    "mixtral8x7b_fp8w8a8_decode_m32": dict(E=8, K=2, H=4096, I=14336, M=32, fmt="fp8", fp8_mode=1),
    # E2M1 expert formats (decoded by the gfx950 scaled-conversion instructions)
    "mixtral8x7b_mxfp4_decode_m32": dict(E=8, K=2, H=4096, I=14336, M=32, fmt="mxfp4"),
    "mixtral8x7b_mxfp4_decode_m128": dict(E=8, K=2, H=4096, I=14336, M=128, fmt="mxfp4"),
    "mixtral8x7b_nvfp4_decode_m128": dict(E=8, K=2, H=4096, I=14336, M=128, fmt="nvfp4"),
    # BASELINE.json configs[4]: GLM-4.5-Air prefill, 8192 tokens (MFMA-bound: roofline in TFLOP/s).  The model's router is
    # sigmoid + score-correction bias through grouped top-k with ONE group (models/glm4_moe.py:190-204; Glm4MoeConfig:
    # n_group = topk_group = 1, norm_topk_prob, routed_scaling_factor 1.0)
    "glm45air_bf16_prefill_m8192": dict(E=128, K=8, H=4096, I=1408, M=8192, fmt="bf16", prefill=True, router=_GLM_ROUTER),
    "glm45air_fp8w8a16_prefill_m8192": dict(E=128, K=8, H=4096, I=1408, M=8192, fmt="fp8", fp8_mode=0, prefill=True, router=_GLM_ROUTER),
    "glm45air_fp8w8a8_prefill_m8192": dict(E=128, K=8, H=4096, I=1408, M=8192, fmt="fp8", fp8_mode=1, prefill=True, router=_GLM_ROUTER),
    "glm45air_int4g128_prefill_m8192": dict(E=128, K=8, H=4096, I=1408, M=8192, fmt="int4", g=128, prefill=True, router=_GLM_ROUTER),
}
HEADLINE = "mixtral8x7b_bf16_decode_m32"
EXTRA_N1 = [# the headline workload under Zipf routing first, in the thermal state the headline itself ran in (after the
            # prefill workload the same kernels measure 1-3 % slower): SURVEY 8d "uniform and Zipf"; methodology
            # benchmarks/kernels/benchmark_moe.py:96-333
            ("mixtral8x7b_bf16_decode_m32", "zipf"),
            "mixtral8x7b_fp8w8a8_decode_m32", "mixtral8x7b_int4g128_decode_m128", "mixtral8x7b_int4g128_fast_decode_m128",
            # BASELINE.json configs[2] says "AWQ-int4": the same layer with ZERO POINTS (asymmetric uint4, LKM_INT4_ZP)
            "mixtral8x7b_int4g128_zp_decode_m128",
            # BASELINE.json configs[4] (the MFMA-bound grouped GEMM) on the uniform-ish routing SURVEY 8d specifies (zero
            # score-correction bias), and on the skewed synthetic bias of rounds 1-5, labelled as such
            "glm45air_fp8w8a8_prefill_m8192", ("glm45air_fp8w8a8_prefill_m8192", "biased"),
            # ... and the path the reference's gpu_prefill actually takes (MOE_BF16 / MOE_FP8 = W8A16: routed_experts.py:1884-1899)
            "glm45air_bf16_prefill_m8192", ("glm45air_bf16_prefill_m8192", "biased"), "glm45air_fp8w8a16_prefill_m8192",
            "mixtral8x7b_int4g128_prefill_m4096",
            # configs[3]'s layer on one GPU under the skewed synthetic bias (174 of 256 experts hit; the uniform default runs
            # below as EXTRA_EP at every N)
            ("dsv3_fp8w8a8_ep_decode_b256", "biased")]
EXTRA_EP = "dsv3_fp8w8a8_ep_decode_b256"
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_PEAK_TF = {"bf16": 2500.0, "fp8": 5000.0}   # dense, MI355X_MICROARCH.md
DUMP_BYTES = 48 << 20       # --dump-outputs: the arrays of all ranks together stay below this
REGIONS_BUDGET_S = 1.0      # the timed region is repeated (--regions) only where all repeats together stay below this


# ------------------------------------------------------------------------------------------ synthetic weights
def make_weights(E_local, first_expert, H, I, dev, fmt, g=128):
    """random-init experts, per-expert seeds so that any EP sharding sees the same model."""
    w13 = torch.empty((E_local, 2 * I, H), dtype=torch.bfloat16, device=dev)
    w2 = torch.empty((E_local, H, I), dtype=torch.bfloat16, device=dev)
    for e in range(E_local):
        gen = torch.Generator(device=dev).manual_seed(7000 + first_expert + e)
        w13[e] = (torch.randn((2 * I, H), generator=gen, device=dev, dtype=torch.float32) / 10).to(torch.bfloat16)
        w2[e] = (torch.randn((H, I), generator=gen, device=dev, dtype=torch.float32) / 10).to(torch.bfloat16)
    return w13, w2


def quantize_int4(w: torch.Tensor, g: int):
    """uint4b8 symmetric group quantisation on the GPU (same recipe as quantize_weights,
    quant_utils.py:642-738; the parity tests check the oracle's version bit-exactly)."""
    E, N, K = w.shape
    wg = w.view(E, N, K // g, g)
    mx, mn = wg.max(dim=-1).values, wg.min(dim=-1).values
    s = torch.maximum((mx / 7).abs(), (mn / -8).abs())
    q = torch.round(wg / s[..., None]).clamp(-8, 7).to(torch.int32) + 8
    q = q.view(E, N, K)
    packed = (q[..., 1::2] * 16 + q[..., ::2]).to(torch.uint8)
    return packed.contiguous(), s.contiguous()


def quantize_fp8_block(w: torch.Tensor, blk: int = 128):
    """128x128 block fp8 (e4m3fn) quantisation on the GPU: scale = amax/448 per block.  Expert by expert: the
    fp32 staging copy of a 256-expert layer would not be worth its 45 GB."""
    E, N, K = w.shape
    nb, kb = -(-N // blk), -(-K // blk)
    q = torch.empty((E, N, K), dtype=torch.uint8, device=w.device)
    s = torch.empty((E, nb, kb), dtype=torch.float32, device=w.device)
    for e in range(E):
        wp = torch.zeros((nb * blk, kb * blk), dtype=torch.float32, device=w.device)
        wp[:N, :K] = w[e].float()
        t = wp.view(nb, blk, kb, blk)
        se = t.abs().amax(dim=(1, 3)).clamp(min=1e-4) / 448.0
        qe = (t / se[:, None, :, None]).view(nb * blk, kb * blk)[:N, :K].contiguous().to(torch.float8_e4m3fn)
        q[e] = qe.view(torch.uint8)
        s[e] = se
    return q, s


_E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def _to_e2m1_codes(v: torch.Tensor) -> torch.Tensor:
    """f32 values (already divided by the block scale) -> E2M1 codes (nearest, saturating at 6)."""
    mid = torch.tensor(_E2M1_MIDPOINTS, device=v.device, dtype=torch.float32)
    code = torch.bucketize(v.abs().contiguous(), mid).to(torch.uint8)
    return code | ((v < 0).to(torch.uint8) << 3)


def quantize_mxfp4(w: torch.Tensor):
    """OCP MXFP4 on the GPU: E8M0 scale 2^(floor(log2(amax)) - 2) per 32 k, E2M1 elements."""
    E, N, K = w.shape
    wg = w.float().view(E, N, K // 32, 32)
    amax = wg.abs().amax(dim=-1).clamp(min=2.0 ** -100)
    e = torch.floor(torch.log2(amax)) - 2
    codes = _to_e2m1_codes(wg / torch.exp2(e)[..., None]).view(E, N, K)
    packed = (codes[..., 1::2] << 4 | codes[..., ::2]).contiguous()
    return packed, (e + 127).clamp(0, 254).to(torch.uint8).contiguous()


def quantize_nvfp4(w: torch.Tensor):
    """NVFP4 on the GPU: per-expert global scale, e4m3fn scale per 16 k, E2M1 elements.  Returns
    (packed, block scales as uint8, per-expert f32 multiplier = 1/global_scale)."""
    E, N, K = w.shape
    wf = w.float()
    gscale = (448.0 * 6.0) / wf.abs().amax(dim=(1, 2)).clamp(min=1e-8)            # [E]
    wg = wf.view(E, N, K // 16, 16)
    sf = (wg.abs().amax(dim=-1) / 6.0 * gscale[:, None, None]).to(torch.float8_e4m3fn)
    sff = sf.float().clamp(min=2.0 ** -9) / gscale[:, None, None]
    codes = _to_e2m1_codes(wg / sff[..., None]).view(E, N, K)
    packed = (codes[..., 1::2] << 4 | codes[..., ::2]).contiguous()
    return packed, sf.view(torch.uint8).contiguous(), (1.0 / gscale).float().contiguous()


def build_engine(ops, wl, E_local, first, dev, **kw):
    """engine over experts [first, first + E_local) of a WORKLOADS entry, built from bf16 master weights in chunks
    of experts (a 256-expert fp8 layer never holds its 22 GB of masters); returns (engine, weight bytes per
    element incl. scales, oracle descriptor kwargs + arrays for the CPU baseline (None above 16 experts), masters
    (bf16 formats only))."""
    fmt, K, H, I = wl["fmt"], wl["K"], wl["H"], wl["I"]
    CH = 8
    parts = []
    for c0 in range(0, E_local, CH):
        n = min(CH, E_local - c0)
        w13, w2 = make_weights(n, first + c0, H, I, dev, fmt)
        if fmt == "int4":
            parts.append((*quantize_int4(w13, wl["g"]), *quantize_int4(w2, wl["g"])))
        elif fmt == "mxfp4":
            parts.append((*quantize_mxfp4(w13), *quantize_mxfp4(w2)))
        elif fmt == "nvfp4":
            a, b, c = quantize_nvfp4(w13)
            d, e, f = quantize_nvfp4(w2)
            parts.append((a, b, d, e, c, f))
        elif fmt == "fp8":
            parts.append((*quantize_fp8_block(w13), *quantize_fp8_block(w2)))
        else:
            parts.append((w13, w2))
        del w13, w2
    cat = [torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(len(parts[0]))]
    del parts
    keep = E_local <= 16
    if fmt == "int4":
        q13, s13, q2, s2 = cat
        g = wl["g"]
        mode = int(wl.get("int4_mode", 0))
        fast = mode == 1
        zkw = {}
        if mode == 2:
            zkw = dict(w13_zp=torch.full(s13.shape, 8, dtype=torch.uint8, device=s13.device),
                       w2_zp=torch.full(s2.shape, 8, dtype=torch.uint8, device=s2.device))
        eng = ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="int4", w13_scale=s13,
                                      w2_scale=s2, group_n=1, group_k=g, int4_mode=mode, **zkw, **kw)
        # the fast mode keeps its group scales as fp32 (4 bytes per row and 128-k block); the zero-point mode (scale, zp) pairs
        return eng, 0.5 + (4.0 if mode else 2.0) / g, dict(wfmt="W_INT4", groupN=1, groupK=g, int4_unrounded=bool(fast),
                                                           w13=q13, w2=q2, s13=s13, s2=s2), None
    if fmt == "mxfp4":
        q13, s13, q2, s2 = cat
        eng = ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="mxfp4", w13_scale=s13,
                                      w2_scale=s2, group_n=1, group_k=32, **kw)
        return eng, 0.5 + 1.0 / 32, dict(wfmt="W_MXFP4", groupN=1, groupK=32, w13=q13, w2=q2, s13=s13, s2=s2), None
    if fmt == "nvfp4":
        q13, s13, q2, s2, g13, g2 = cat
        eng = ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="nvfp4", w13_scale=s13,
                                      w2_scale=s2, group_n=1, group_k=16, w13_global_scale=g13,
                                      w2_global_scale=g2, **kw)
        return eng, 0.5 + 1.0 / 16, dict(wfmt="W_NVFP4", groupN=1, groupK=16, w13=q13, w2=q2, s13=s13, s2=s2,
                                         gs13=g13, gs2=g2), None
    if fmt == "fp8":
        q13, s13, q2, s2 = cat
        a8 = bool(wl.get("fp8_mode", 0))
        eng = ops.RoutedExpertsEngine(q13, q2, top_k=K, act_dtype=torch.bfloat16, fmt="fp8", w13_scale=s13,
                                      w2_scale=s2, group_n=128, group_k=128, fp8_mode=wl.get("fp8_mode", 0), **kw)
        oi = dict(wfmt="W_FP8", groupN=128, groupK=128, w8a8=a8, round_gemm1=a8, w13=q13, w2=q2, s13=s13,
                  s2=s2) if keep else None
        return eng, 1.0 + 4.0 / (128 * 128), oi, None
    w13, w2 = cat
    eng = ops.RoutedExpertsEngine(w13, w2, top_k=K, act_dtype=torch.bfloat16, fmt="bf16", **kw)
    return eng, 2.0, (dict(wfmt="W_BF16", groupN=0, groupK=0, w13=w13, w2=w2) if keep else None), (w13, w2)


# ------------------------------------------------------------------------------------------ CPU baselines
def host_info():
    """what SURVEY 8d asks to state next to a CPU number: logical CPUs, sockets, NUMA nodes of this box"""
    info = {"nproc": os.cpu_count() or 1}
    try:
        ids = {ln.split(":")[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("physical id")}
        info["sockets"] = max(1, len(ids))
        model = [ln.split(":")[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")]
        if model:
            info["cpu"] = model[0]
    except OSError:
        pass
    try:
        info["numa_nodes"] = len([p for p in Path("/sys/devices/system/node").glob("node[0-9]*")])
    except OSError:
        pass
    try:
        info["affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    return info


def time_reference_kernel(w13, w2, x, tw, ids, thread_cands, seconds, gpu_out):
    """cpu_baseline kind "reference": oracle/_ref (the reference's in-tree CPU fused-MoE kernel) on this host."""
    from oracle import ref
    if not ref.available():
        return None
    ref.load()
    p13, p2 = ref.prepack(w13.cpu()), ref.prepack(w2.cpu())
    xc, twc, idc = x.cpu(), tw.cpu(), ids.cpu()
    ref.set_threads(thread_cands[0])
    ref.fused_moe(xc, p13, p2, twc, idc)                            # untimed first pass
    best_t, best_c, probe = None, thread_cands[0], {}
    for c in thread_cands:                                          # same team-size probe as for the port
        ref.set_threads(c)
        ref.fused_moe(xc, p13, p2, twc, idc)                        # untimed: a larger team spawns and binds its threads in this pass
        ts = []                                                     # median of 5: one timed pass right after a resize read 158 ms at
        for _ in range(5):                                          # 16 threads on one box and ended the probe at 8 (44 ms instead of
            c0 = time.perf_counter()                                # 15); the minimum of two picked a 128-thread team that runs 7 ms
            ref.fused_moe(xc, p13, p2, twc, idc)                    # now and then and 200 ms most of the time
            ts.append(time.perf_counter() - c0)
        tc = float(np.median(ts))
        probe[str(c)] = round(tc * 1e3, 2)
        if best_t is None or tc < best_t:
            best_t, best_c = tc, c
        if tc > 3 * best_t and c >= 64:                             # (8 ... 64 are always measured)
            break
    ref.set_threads(best_c)
    # median of >= 5 timed passes (the mean of a time-boxed loop moved 12 -> 25 ms per step between sessions: VERDICT r3)
    times, out = [], None
    while len(times) < 5 or (sum(times) < seconds and len(times) < 200):
        c0 = time.perf_counter()
        out = ref.fused_moe(xc, p13, p2, twc, idc)
        times.append(time.perf_counter() - c0)
    n, t_cpu = len(times), sum(times)
    med = float(np.median(times))
    # ... and the all-cores figure SURVEY 8d asks for (one warm pass + one timed pass: it can be 10-50x slower)
    all_cores = None
    ncpu = max(thread_cands)
    if ncpu != best_c:
        ref.set_threads(ncpu)
        ref.fused_moe(xc, p13, p2, twc, idc)
        c0 = time.perf_counter()
        ref.fused_moe(xc, p13, p2, twc, idc)
        all_cores = {"cores": ncpu, "ms_per_step": round((time.perf_counter() - c0) * 1e3, 2)}
        ref.set_threads(best_c)
    o = out.float().numpy()
    err = float(np.abs(gpu_out - o).max() / max(1e-9, np.abs(o).max()))
    return {"value": round(x.size(0) / med, 2), "unit": "tokens/s", "cores": best_c, "kind": "reference",
            "ms_per_step": round(med * 1e3, 2), "ms_per_step_stat": "median", "passes": n,
            "ms_per_step_min_max": [round(min(times) * 1e3, 2), round(max(times) * 1e3, 2)],
            "binding": {"KMP_AFFINITY": os.environ.get("KMP_AFFINITY")}, "all_cores": all_cores,
            "max_rel_err_gpu_vs_cpu": err, "n": n, "t": t_cpu,
            "team_probe_ms": probe}


def cpu_baseline(name, wl, oracle_in, masters, x, tw, ids, gpu_out, seconds):
    """the CPU oracle (port of the reference algorithm) and, for 16-bit experts, the reference's own in-tree CPU
    kernel (oracle/_ref) on the same inputs and this box's host cores"""
    from oracle import oracle as orc
    E, H, I, M = wl["E"], wl["H"], wl["I"], x.size(0)
    twn, idn = tw.cpu().numpy(), ids.cpu().numpy()
    xb = x.cpu().view(torch.int16).numpy().view(np.uint16)

    def _np(t):
        t = t.cpu()
        return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()
    oi = dict(oracle_in)
    d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=orc.BF16, wfmt=getattr(orc, oi.pop("wfmt")), groupN=oi.pop("groupN"),
                    groupK=oi.pop("groupK"), w8a8=oi.pop("w8a8", False), round_gemm1=oi.pop("round_gemm1", False),
                    int4_unrounded=oi.pop("int4_unrounded", False))
    cargs = {k_: _np(v) for k_, v in oi.items()}
    ref = orc.moe(d, x=xb, ids=idn, tw=twn, **cargs)            # untimed first pass (page-in)
    # The host may expose more logical CPUs than the container can actually run (measured on the
    # bench box: 32 threads 49 ms, 64 threads 77 ms, 128 threads 137 ms, 256 threads 960 ms per
    # step), so the team size is picked by a short probe; `cores` reports the size used.
    ncpu = os.cpu_count() or 1
    cands = sorted({c for c in (8, 16, 32, 64, 128, ncpu) if c <= ncpu})
    best_t, best_c, probe = None, cands[0], {}
    for c in cands:
        orc.set_threads(c)
        orc.moe(d, x=xb, ids=idn, tw=twn, **cargs)                  # untimed: the resized team's first pass
        ts = []
        for _ in range(3):
            c0 = time.perf_counter()
            orc.moe(d, x=xb, ids=idn, tw=twn, **cargs)
            ts.append(time.perf_counter() - c0)
        tc = float(np.median(ts))
        probe[str(c)] = round(tc * 1e3, 2)
        if best_t is None or tc < best_t:
            best_t, best_c = tc, c
        if tc > 3 * best_t and c >= 64:
            break
    orc.set_threads(best_c)
    n, t_cpu = 0, 0.0
    while n < 2 or (t_cpu < seconds and n < 200):
        c0 = time.perf_counter()
        ref = orc.moe(d, x=xb, ids=idn, tw=twn, **cargs)
        t_cpu += time.perf_counter() - c0
        n += 1
    err = float(np.abs(gpu_out - ref).max() / max(1e-9, np.abs(ref).max()))
    cpu = {"value": round(M / (t_cpu / n), 2), "unit": "tokens/s", "cores": orc.num_threads(), "kind": "port",
           "sample": f"{n} full {name} layer passes (M={M}) through oracle/lkm_oracle.c, "
                     f"{t_cpu:.1f} s of CPU work; lk_moe itself is a closed binary absent from the reference tree",
           "ms_per_step": round(t_cpu / n * 1e3, 2), "max_rel_err_gpu_vs_cpu": err, "host": host_info(),
           # one pass per candidate team size (threads -> ms); the probe stops once a size is 3x slower than the best:
           # the host exposes more logical CPUs than the container runs well (SURVEY 8d asks for "all host cores":
           # these timings are why `cores` is smaller)
           "team_probe_ms": probe}
    # The reference's OWN in-tree CPU fused-MoE kernel (csrc/cpu/cpu_fused_moe.cpp, compiled into oracle/_ref
    # where /root/reference exists; 16-bit experts only) on the same inputs and host cores: when it loads it
    # IS the cpu_baseline ("reference") and the port's figure moves to cpu_baseline["port"].
    if wl["fmt"] == "bf16" and masters is not None:
        try:
            cpu_ref = time_reference_kernel(masters[0], masters[1], x, tw, ids, cands, seconds, gpu_out)
        except Exception as e:
            print(f"[bench] oracle/_ref unavailable ({e}); cpu_baseline is the port", file=sys.stderr)
            cpu_ref = None
        if cpu_ref is not None:
            cpu_ref["sample"] = (f"{cpu_ref.pop('n')} full {name} layer passes (M={M}) through the reference's "
                                 f"csrc/cpu/cpu_fused_moe.cpp (AVX-512 'vec' micro-kernels, oracle/_ref), "
                                 f"{cpu_ref.pop('t'):.1f} s of CPU work")
            cpu_ref["host"] = cpu.pop("host")
            cpu_ref["port"] = cpu
            cpu = cpu_ref
    return cpu


# ------------------------------------------------------------------------------------------ one workload
def mfma_peak_tf(wl):
    """dense MFMA peak (TFLOP/s) of the instruction the format's kernels multiply with: fp8 x fp8 runs on the MX-scaled
    fp8 MFMA (5 PF); every other format is decoded to the 16-bit activation dtype in registers (2.5 PF)"""
    return MFMA_PEAK_TF["fp8" if (wl["fmt"] == "fp8" and wl.get("fp8_mode")) else "bf16"]


def kernel_source_hash() -> str:
    """hash of the HIP sources the kernels are built from (profiles/hbm_traffic.json records the one its PMC pass ran on)"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted((ROOT / "lvllm_amd" / "csrc").glob("*.h*")):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def prefill_like(wl) -> bool:
    return bool(wl.get("prefill"))


def roof_fields(flops, bytes_, ms, peak_tf):
    """the two rooflines of one kernel side by side (BASELINE.json's metric names the MFMA roofline, the decode
    kernels are HBM-bound): achieved TFLOP/s and GB/s, their fractions of the dense MFMA peak and of the 8 TB/s HBM
    peak, and the fraction of the binding roof min(MFMA peak, arithmetic intensity x HBM peak)"""
    tf = flops / (ms * 1e-3) / 1e12
    gbs = bytes_ / (ms * 1e-3) / 1e9
    ai = flops / max(1.0, bytes_)
    roof_tf = min(peak_tf, ai * HBM_PEAK_GBS / 1e3)
    return {"tflops": round(tf, 2), "mfma_peak_tflops": peak_tf, "mfma_frac": round(tf / peak_tf, 4),
            "GBps": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
            "arithmetic_intensity_flop_per_byte": round(ai, 2), "roof_tflops": round(roof_tf, 2),
            "roof_bound": "mfma" if roof_tf >= peak_tf else "hbm", "frac_of_roof": round(tf / roof_tf, 4)}


def dump_outputs(dirname, arrays, rank, world):
    """--dump-outputs: what the last timed step handed its caller, one float32 DIR/<name>.npy per array (a rank of a
    multi-GPU run adds _rank<r> to the name).  Where that would pass DUMP_BYTES over all ranks, the same seeded sample of
    rows of every array is kept and its row numbers go to sampled_rows.npy."""
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    tag = f"_rank{rank}" if world > 1 else ""
    rows = next(iter(arrays.values())).size(0)
    row_bytes = sum(t[0].numel() for t in arrays.values()) * 4
    keep = None
    if rows * row_bytes > DUMP_BYTES // world:
        keep = np.sort(np.random.default_rng(0).choice(rows, DUMP_BYTES // world // row_bytes, replace=False))
        np.save(d / f"sampled_rows{tag}.npy", keep.astype(np.float64))
    for k_, t in arrays.items():
        if keep is not None:
            t = t[torch.from_numpy(keep).to(t.device)]
        np.save(d / f"{k_}{tag}.npy", t.float().cpu().numpy())


def run_workload(name, args, ctx, *, steps, warmup, with_cpu, full, force_ep=False, routing=None, dump_dir=None):
    """times `steps` steps of one WORKLOADS entry on this rank set; returns the result dict on rank 0 (None
    elsewhere).  Every rank must call it with the same arguments (it contains collectives when world > 1).
    full (bench.py --full): also the longer run of the same step, the per-kernel roofline pass and, with_cpu, the CPU
    baselines -- runs of their own after the timed steps, which a plain run leaves out (`roofline`: null)."""
    from lvllm_amd import ops
    from lvllm_amd.ep import ExpertParallelExperts
    world, rank, dev = ctx["world"], ctx["rank"], ctx["dev"]
    wl = WORKLOADS[name]
    E, K, H, I, fmt = wl["E"], wl["K"], wl["H"], wl["I"], wl["fmt"]
    if "M_global" in wl:
        if wl["M_global"] % world:
            return None
        M, scaling = wl["M_global"] // world, "strong"
    else:
        M, scaling = wl["M"], "weak"
    if args.batch_per_gpu and name == args.workload:      # (development: the same experts at another batch size)
        M = args.batch_per_gpu
    if E % world:
        return None
    use_ep = world > 1 or force_ep
    E_local, first = E // world, rank * (E // world)
    eng, bpe, oracle_in, masters = build_engine(ops, wl, E_local, first, dev, max_num_seqs=max(256, M * world),
                                                max_batch_size=max(8192, M), num_processes=world, process_id=rank)
    if args.autotune:
        # opt-in: the plan of each decode-sized step shape is picked by the engine's first-call micro-autotune (2-7 candidate
        # plans timed on the step's own inputs during the warm-up steps; the choice is in config.geometry: "autotuned: ...").
        # An expert-parallel engine takes value 2 and the ranks agree on the plans before the capture (ep.agree_tuned_plans).
        eng.engine.set_tuning(autotune=2 if world > 1 else 1)
    if args.tune:
        eng.engine.set_tuning(**{k: int(v) for k, v in (kv.split("=") for kv in args.tune.split(","))})

    # synthetic inputs (seed 7): x = randn/10, router logits = randn
    gen = torch.Generator(device=dev).manual_seed(7 + rank)
    x = (torch.randn((M, H), generator=gen, device=dev) / 10).to(torch.bfloat16)
    logits = torch.randn((M, E), generator=gen, device=dev, dtype=torch.float32)
    routing = routing or args.routing
    if routing == "nobias":    # round-5 name of what is now the default of the bias routers
        routing = "uniform"
    if routing == "zipf":      # log-popularity bias: p(e) ~ 1/(e+1)
        logits = logits + torch.log(1.0 / torch.arange(1, E + 1, device=dev, dtype=torch.float32))[None, :]
    rt = wl.get("router", dict(kind="softmax"))
    bias = None
    if rt.get("bias"):
        # The sigmoid + score-correction-bias routers (GLM-4.5-Air, DeepSeek-V3).  A model's bias is LEARNED to balance the
        # load, so "uniform" (randn logits, uniform-ish routing) and "zipf" run these routers with a ZERO bias.
        # "biased" adds the synthetic N(0, 0.1) bias rounds 1-5 used by default and mislabelled "uniform": on randn logits it
        # SKEWS the routing (GLM workload: 3 of 128 experts get no row, the busiest 4469 of 65 536 = 8.7 x the mean; DSv3:
        # 174 of 256 experts hit -- profiles/r05_a8w_uniform_items_probe.log); it stays as a separately labelled skewed variant.
        bias = torch.zeros((E,), device=dev)
        if routing == "biased":
            bias = torch.randn((E,), generator=torch.Generator(device=dev).manual_seed(99), device=dev) * 0.1

    def route():
        if rt["kind"] == "grouped":
            return ops.grouped_topk(x, logits, K, True, rt["n_group"], rt["topk_group"], rt["scoring"],
                                    rt["routed_scaling"], bias)
        return ops.topk_softmax(logits, K, True)
    prefill = bool(wl.get("prefill"))
    out = torch.empty((M, H), dtype=torch.bfloat16 if prefill else torch.float32, device=dev)
    ep = None
    last = {}       # what the latest step() handed back (a captured step: the graph's own tensors, rewritten by every replay)
    if not use_ep:
        if prefill:
            def step():
                tw, ids = route()
                last["ret"] = (eng.forward_rows(x, tw, ids, out=out), tw, ids)
        else:
            # decode: routing + scatter metadata in one launch (lkm_forward_routed; --tune fuse=-1 gives the five-launch
            # step back; same bits)
            fl = dict(scoring_func=rt.get("scoring", "softmax"), e_score_correction_bias=bias, out=out)
            if rt["kind"] == "grouped":
                fl.update(num_expert_group=rt["n_group"], topk_group=rt["topk_group"],
                          routed_scaling_factor=rt["routed_scaling"])

            def step():
                last["ret"] = eng.forward_logits(x, logits, K, True, **fl)
    else:
        def local_compute(rows, lids, ws, dt, valid_den=None):
            # (a2a mode hands over ep x capacity token records of which ~1/ep carry local ids and says so: valid_den)
            return eng.forward_rows(rows, ws, lids, out_dtype=dt, valid_den=valid_den)
        # group-limited routers (DeepSeek-V3 / GLM): a token visits <= topk_group ranks, so the record capacity per
        # destination is the group-limited estimate -- slack 1.25 + collective fallback in eager steps, slack 1.75 in the
        # captured step (lvllm_amd/ep.py); the overflow counter is read after the timed replays (config.ep_overflow_tokens)
        rg = (rt["n_group"], rt["topk_group"]) if rt["kind"] == "grouped" and rt["n_group"] > 1 else None
        ep = ExpertParallelExperts(local_compute, E, H, mode=args.ep_mode, routing_groups=rg,
                                   return_dtype=torch.float32 if args.ep_return == "f32" else None)

        def step():
            tw, ids = route()
            last["ret"] = (ep.forward(x, tw, ids, force_collectives=True, out=out), tw, ids)

    def barrier():
        if ctx["dist"]:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warm-up (also creates the communicator and the persistent exchange buffers before any capture)
    for _ in range(max(1, warmup)):
        step()
    barrier()
    if args.autotune and world > 1:
        from lvllm_amd.ep import agree_tuned_plans
        agree_tuned_plans([eng.engine])
    launch, graph = "eager", None
    wd = ctx.get("wd")
    if wd is not None and not args.no_graph:
        # the same K steps launched eagerly first: a complete measurement to fall back on should the captured step
        # (collectives inside a hipGraph) not come back on this machine
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        barrier()
        te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        e_dt = float(te.item())
        wd.arm(180.0, {
            "metric": "moe_layer_decode_tokens_per_s", "value": round(M * world / (e_dt / steps), 1), "unit": "tokens/s",
            "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": round(e_dt / steps * 1e3, 4),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": fmt, "data": "synthetic",
            "config": {"workload": name, "experts": E, "experts_per_gpu": E_local, "top_k": K, "hidden": H,
                       "intermediate": I, "batch_per_gpu": M, "global_batch": M * world,
                       "parallelism": "single" if not use_ep else f"ep{world}-{args.ep_mode}", "launch": "eager"},
            "roofline": None, "cpu_baseline": None} if name == args.workload else wd.fallback,
            f"graph capture / replay of workload {name}")
    if not args.no_graph:
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream().wait_stream(s)
            barrier()
            graph = torch.cuda.CUDAGraph()
            # thread_local: with a process group alive, c10d's watchdog thread queries events while this thread
            # captures; in the default (global) mode such a call from ANY thread invalidates the capture -- seen as
            # hipErrorStreamCaptureInvalidated in about one of three test-suite runs of the one-rank RCCL step
            with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local" if ctx["dist"] else "global"):
                step()
            graph.replay()
            barrier()
            launch = "hipgraph"
        except Exception as e:  # capture is an optimisation of the launch path only
            print(f"[bench] graph capture unavailable ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
            graph = None
    if ctx["dist"]:
        # all ranks must agree on the launch path (a rank replaying a graph against a rank launching eagerly is
        # still the same sequence of collectives, but the timing would mix two things)
        flag = torch.tensor([1 if graph is not None else 0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            graph, launch = None, "eager"
    run = (lambda: graph.replay()) if graph is not None else step

    # ---- pre-roll: untimed steps through the launch path that is about to be timed, so that the GPU has been busy for
    # ~30 ms when it reaches the opening barrier.  After an idle stretch (graph capture: milliseconds of host work) the
    # clocks need about that long to settle, and a 20-step region of a 0.25-0.45 ms step would otherwise measure the ramp:
    # Mixtral bf16 M=32 at K = 20: 450 us without, 432-437 with 50 steps of pre-roll, 432 over 2000 steps; int4 M=128:
    # 292 against 246 (profiles/r03_timed_region_length.log).  At least W steps, at most 200; the count is reported
    # (`config.preroll_steps`).  The timed region itself is untouched: exactly K steps between two barriers.
    preroll = 0
    if os.environ.get("LKM_BENCH_NO_PREROLL") != "1":
        barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            run()
        barrier()
        est = max((time.perf_counter() - t0) / 3, 1e-5)
        preroll = int(min(200, max(warmup, 1, math.ceil(0.03 / est))))
        if ctx["dist"]:      # (every rank the same count: the steps contain collectives)
            pr = torch.tensor([preroll], device=dev)
            dist.all_reduce(pr, op=dist.ReduceOp.MAX)
            preroll = int(pr.item())
        for _ in range(preroll):
            run()
    # ---- timed regions: each one exactly `steps` steps, barrier + synchronize on both sides, MAX over ranks.
    # R = 5 regions back to back and the MEDIAN region is the line's value (all five are reported, `timed_regions_ms`):
    # the pool's boxes freeze the GPU queue for ~86 ms now and then (tools/prof_rep_stall.py, profiles/r05_prof_rep_stall.log:
    # twice in ~2 s of launches on one box -- the event that turned round 4's driver test run red); one such event inside a
    # 9 ms region of 20 steps would report a tenth of the throughput.  --regions 1 gives the single region back.  The
    # repeats are there for SHORT regions: when R times the first region would pass REGIONS_BUDGET_S the first one stands
    # alone (its reduced time is the same on every rank, so the ranks decide alike), and a run whose --steps fill a second
    # times exactly those steps, once.
    regions = []
    for _ in range(max(1, args.regions)):
        if regions and regions[0] * args.regions > REGIONS_BUDGET_S:
            break
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if ctx["dist"]:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        regions.append(float(t.item()))
    dt = float(np.median(regions))
    ms_per_step = dt / steps * 1e3
    tokens_per_s = M * world / (dt / steps)
    if wd is not None:
        wd.disarm()
    if dump_dir:
        dump_outputs(dump_dir, dict(zip(("out", "topk_weights", "topk_ids"), last["ret"])), rank, world)

    # ---- the same step over a longer run (reported next to the line's value, never instead of it): right after the
    # synchronisation that opens a timed region the GPU clocks ramp for a few milliseconds, which a 20-step region of a
    # 0.44 ms step carries in full (Mixtral bf16 M=32, one box: 450 us at K = 20, 436 at K = 200, 432 at K = 2000:
    # profiles/r03_timed_region_length.log)
    long_run = None
    LONG = 400
    if full and steps < LONG and not prefill_like(wl) and not use_ep:
        barrier()
        t0 = time.perf_counter()
        for _ in range(LONG):
            run()
        barrier()
        long_run = {"steps": LONG, "ms_per_step": round((time.perf_counter() - t0) / LONG * 1e3, 4),
                    "what": "the same captured step, one longer timed region (the clock ramp after the opening "
                            "synchronisation weighs less); `value` above is the K-step region the contract asks for"}

    # ---- optional: cold-cache variant.  Not part of the timed steps above.
    cold_ms = None
    if args.flush_cache and rank == 0 and not use_ep:     # EP steps are collective: every rank would have to join
        flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        n_cold = min(steps, 50)
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(n_cold)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(n_cold)]
        for i in range(n_cold):
            flush.fill_(i & 0xFF)
            starts[i].record()
            run()
            ends[i].record()
        torch.cuda.synchronize()
        cold_ms = sum(a.elapsed_time(b) for a, b in zip(starts, ends)) / n_cold
        del flush

    # ---- dominant-kernel roofline: GEMM1 duration from HIP events on the launch stream (rank 0's engine)
    res = None
    if full:
        tw, ids = route()
        lids = ids
        if world > 1:
            lids = torch.where((ids >= first) & (ids < first + E_local), ids - first, torch.full_like(ids, -1))

    def measure_roofline():
        # each GEMM is launched PROF_REP times back to back between its two events and the interval divided
        # (lkm_set_tuning "prof_rep"): a single launch between two events also times the event packets,
        # ~10 us on top of the kernel time rocprofv3 reports for the same launch
        PROF_REP = 8
        pout = torch.empty((M, H), dtype=torch.float32, device=dev)
        eng.engine.set_tuning(prof_rep=PROF_REP)
        eng.engine.set_profiling(True)
        acc = {"sort": [], "gemm1": [], "gemm2": [], "combine": []}
        reps = 30 if not prefill else 7
        if not use_ep and not prefill:      # the timed step's own launches: "sort" = router + sort
            def prof_call():
                eng.forward_logits(x, logits, K, True, **{**fl, "out": pout})
        else:
            def prof_call():
                eng.decode(x, tw, lids, out=pout)
        for _ in range(3):
            prof_call()
        for _ in range(reps):
            prof_call()
            p = eng.engine.get_profile()
            for k_ in acc:
                acc[k_].append(p[k_])
        kernels = eng.engine.last_kernels()            # the GEMM kernels these launches really were (lkm_last_kernels)
        plan = eng.engine.describe().split(" | ", 1)[-1]
        eng.engine.set_profiling(False)
        eng.engine.set_tuning(prof_rep=0)
        # MEDIAN over the profiled calls (round 4: the driver's box once put an 86 ms stall between eight back-to-back
        # launches of an 8 us kernel; a mean would carry such an outlier into the roofline); min / max are reported
        prof_ms = {k_: float(np.median(v)) for k_, v in acc.items()}
        prof_range = {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in acc.items() if k_.startswith("gemm")}
        e_act = int(torch.unique(lids[lids >= 0]).numel())
        rows = int((lids >= 0).sum().item())
        per_e = torch.bincount(lids[lids >= 0].flatten().long(), minlength=E_local)
        g1_bytes = e_act * 2 * I * H * bpe                           # algorithmic weight bytes of GEMM1 (bpe incl. scales)
        layer_flops = 6.0 * rows * H * I
        layer_bytes = e_act * 3 * I * H * bpe
        g1_ms = max(prof_ms["gemm1"], 1e-6)
        g1_flops = 4.0 * rows * H * I                                # gate + up projections of every routed row
        both = roof_fields(g1_flops, g1_bytes, g1_ms, mfma_peak_tf(wl))
        # roofline.traffic: the FETCH_SIZE pass of THIS kernel under THIS plan (tools/update_hbm_traffic.py records the
        # kernel name from lkm_last_kernels and the plan string), or null with the reason -- never another plan's bytes
        g1_kernel = "+".join(kernels.get("gemm1", [])) or None
        traffic, stale, tnote = None, None, "no FETCH pass on file for this workload"
        tf = ROOT / "profiles" / "hbm_traffic.json"
        if tf.exists():
            try:
                tj = json.loads(tf.read_text())
                ent = tj.get(name if routing == "uniform" else f"{name}@{routing}", {})
                stale = tj.get("kernel_source_hash") != kernel_source_hash()
                if ent.get("gemm1_bytes_per_launch") is not None:
                    if ent.get("gemm1_kernel") != g1_kernel:
                        tnote = f"FETCH pass on file is of another kernel ({ent.get('gemm1_kernel')})"
                    elif ent.get("plan") != plan:
                        tnote = "FETCH pass on file is of another launch plan"
                    else:
                        traffic, tnote = ent["gemm1_bytes_per_launch"], None
            except Exception as e:
                tnote = f"profiles/hbm_traffic.json unreadable ({type(e).__name__})"
        tsrc = (tnote if traffic is None else
                "profiles/hbm_traffic.json: rocprofv3 --pmc FETCH_SIZE pass of this workload, kernel and plan "
                "(tools/update_hbm_traffic.py), gfx950-corrected (x2); traffic_stale: kernel sources changed since")
        if prefill:     # MFMA-bound regime: the roofline of the dominant kernel is flops against the dense MFMA peak
            peak = mfma_peak_tf(wl)
            ach = g1_flops / (g1_ms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "kernel": g1_kernel, "achieved": round(ach, 1), "peak": peak,
                        "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": tsrc,
                        "traffic_stale": stale, "algorithmic_bytes": g1_bytes, "algorithmic_flops": g1_flops}
            # the second GEMM of the step against the same peak (2 * rows * I * H flops), and what the GEMM1 launch also does
            g2_ms = max(prof_ms.get("gemm2", 0.0), 1e-6)
            roofline["gemm2"] = {"achieved": round(2.0 * rows * H * I / (g2_ms * 1e-3) / 1e12, 1), "unit": "TFLOP/s",
                                 "frac": round(2.0 * rows * H * I / (g2_ms * 1e-3) / 1e12 / peak, 4)}
            if wl.get("fp8_mode") == 1 and wl.get("fmt") == "fp8":
                roofline["kernel_includes"] = ("gated SiLU and the 1 x 128 fp8 quantisation of the intermediate in GEMM1's epilogue "
                                               "(a separate 37-us pass until late round 3); the GEMM2 bracket holds GEMM2 only")
        else:
            achieved = g1_bytes / (g1_ms * 1e-3) / 1e9               # (a rank whose experts got no row: 0)
            roofline = {"bound": "hbm", "kernel": g1_kernel, "achieved": round(achieved, 1),
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                        "traffic": traffic, "traffic_source": tsrc, "traffic_stale": stale, "algorithmic_bytes": g1_bytes}
        roofline.update(both)       # mfma_frac, hbm_frac, roof = min(MFMA, AI x HBM), frac_of_roof: both rooflines, always
        step_fl = roof_fields(layer_flops, layer_bytes, ms_per_step, mfma_peak_tf(wl))
        roofline.update({
            "step": {"mfma_frac": step_fl["mfma_frac"], "hbm_frac": step_fl["hbm_frac"], "frac_of_roof": step_fl["frac_of_roof"],
                     "roof_bound": step_fl["roof_bound"],
                     "what": "the whole layer step (router, scatter, GEMM1, GEMM2, combine) against the same two peaks"},
            "layer": {"routed_rows": rows, "experts_hit": e_act, "rows_per_expert_min_max": [int(per_e.min()), int(per_e.max())],
                      "weight_bytes": layer_bytes, "flops": layer_flops,
                      "GBps_over_step": round(layer_bytes / (ms_per_step * 1e-3) / 1e9, 1),
                      "TFLOPs_over_step": round(layer_flops / (ms_per_step * 1e-3) / 1e12, 2)},
            "kernel_ms": {k_: round(v, 4) for k_, v in prof_ms.items()},
            "kernel_ms_min_max": prof_range, "gemm2_kernel": "+".join(kernels.get("gemm2", [])) or None, "plan": plan,
            "timing": f"HIP events on the launch stream around {PROF_REP} back-to-back launches, / {PROF_REP}; median of {reps} calls"
                      + (" (rank 0's engine on rank 0's own routed rows)" if world > 1 else "")})
        return roofline
    if rank == 0:
        roofline = measure_roofline() if full else None
        res = {"workload": name, "value": round(tokens_per_s, 1), "unit": "tokens/s", "ms_per_step": round(ms_per_step, 4),
               "steps": steps, "scaling": scaling, "timed_regions_ms": [round(r * 1e3, 3) for r in regions],
               "dtype": {"bf16": "bf16", "int4": "int4-w/bf16-act" + {0: "", 1: " (fast mode: scale on fp32 partial sums)", 2: " (zero points: T((q - zp) s))"}[int(wl.get("int4_mode", 0))],
                         "mxfp4": "mxfp4-w/bf16-act",
                         "nvfp4": "nvfp4-w/bf16-act",
                         "fp8": "fp8-w/" + ("fp8-act" if wl.get("fp8_mode") else "bf16-act")}[fmt],
               "config": {"workload": name, "experts": E, "experts_per_gpu": E_local, "top_k": K, "hidden": H,
                          "intermediate": I, "batch_per_gpu": M, "global_batch": M * world,
                          "router": rt["kind"] if rt["kind"] == "softmax" else
                          f"grouped {rt['scoring']}+bias top-{K} of {rt['topk_group']}/{rt['n_group']} groups x{rt['routed_scaling']}",
                          "routing": routing,
                          "parallelism": "single" if not use_ep else f"ep{world}-{args.ep_mode}",
                          "launch": launch, "preroll_steps": preroll, "autotune": bool(args.autotune),
                          "geometry": eng.engine.describe()},
               "roofline": roofline}
        if ep is not None and args.ep_mode == "a2a":
            rb = 4 if args.ep_return == "f32" else 2
            captured = launch != "eager"
            res["config"]["exchange"] = dict(ep.wire_bytes(M, K, ret_bytes=rb, capturing=captured),
                                             granularity="token records [x | ids | weights]; capacity = tokens per rank, or the "
                                                         "group-limited estimate (slack 1.25 eager + fallback / 1.75 captured) "
                                                         "when the router is group-limited",
                                             return_dtype="fp32" if rb == 4 else "bf16",
                                             # records that did not fit a destination's slots during this workload's steps
                                             # (a captured step cannot branch on it: non-zero = re-run eagerly)
                                             overflow_tokens=ep.overflow_count())
        if cold_ms is not None:
            res["ms_per_step_cold"] = round(cold_ms, 4)     # events around each step, caches evicted before it
        if long_run is not None:
            res["long_run"] = long_run
        if with_cpu and world == 1 and oracle_in is not None:
            gpu_out = eng.decode(x, tw, ids).cpu().numpy()
            res["cpu_baseline"] = cpu_baseline(name, wl, oracle_in, masters, x, tw, ids, gpu_out, args.cpu_seconds)
    barrier()
    del graph, eng, ep, oracle_in, masters
    gc.collect()
    torch.cuda.empty_cache()
    return res


# ------------------------------------------------------------------------------------------ launch
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class Watchdog:
    """Multi-rank runs only.  The captured expert-parallel step (RCCL collectives inside a hipGraph) and the extra
    workloads have run on ONE rank before the driver's N > 1 runs; if a step of them never completes there, rank 0 still
    prints the best line it already holds (the eager-launch timing of the same K steps, or the finished headline
    line) and every rank leaves, instead of the whole run timing out with nothing."""

    def __init__(self, rank: int):
        import threading
        self.rank, self.deadline, self.fallback, self.what = rank, None, None, ""
        self._lock = threading.Lock()
        threading.Thread(target=self._loop, daemon=True).start()

    def arm(self, seconds: float, fallback: dict | None, what: str) -> None:
        with self._lock:
            self.deadline, self.fallback, self.what = time.monotonic() + seconds, fallback, what

    def disarm(self) -> None:
        with self._lock:
            self.deadline = None

    def _loop(self) -> None:
        while True:
            time.sleep(1.0)
            with self._lock:
                fired = self.deadline is not None and time.monotonic() > self.deadline
                fb, what = self.fallback, self.what
            if fired:
                print(f"[bench] rank {self.rank}: {what} did not complete in time", file=sys.stderr, flush=True)
                if self.rank == 0 and fb is not None:
                    fb = dict(fb)
                    fb["note"] = f"{what} did not complete; this line is what was measured before it"
                    print(json.dumps(fb), flush=True)
                else:
                    time.sleep(3.0)         # let rank 0 write its line first
                sys.stdout.flush()
                os._exit(0 if fb is not None else 3)


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU
    (the reference's tests spawn their ranks themselves too, tests/kernels/moe/parallel_utils.py:52-118)."""
    have = torch.cuda.device_count()
    if have < n:
        print(f"bench.py: --gpus {n} but only {have} GPU(s) visible", file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default=HEADLINE, choices=list(WORKLOADS))
    ap.add_argument("--ep-mode", default="a2a", choices=["a2a", "ar"])
    ap.add_argument("--ep-return", default="bf16", choices=["bf16", "f32"],
                    help="dtype of the partial rows on the return all-to-all (bf16 = the activation dtype)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--force-ep", action="store_true", help="run the expert-parallel data path even with one rank (plumbing check)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also: the per-kernel roofline pass, a longer run of the same step, the CPU "
                         "baselines, the extra workloads and the --full-out side file (a plain run times the steps and prints "
                         "the line, with `roofline` and `cpu_baseline` null)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step returned (out, topk_weights, topk_ids) as float32 DIR/<name>.npy; the "
                         "inputs are seeded, so two builds run with the same arguments can be compared array by array")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baselines out")
    ap.add_argument("--no-extras", action="store_true", help="with --full: time the headline workload only")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget (s) for each CPU baseline sample (reference kernel, port)")
    ap.add_argument("--routing", default="uniform", choices=["uniform", "zipf", "biased", "nobias"],
                    help="router logits: randn (uniform-ish; the sigmoid + bias routers run a ZERO score-correction bias) or "
                         "randn + Zipf(s=1) expert popularity (SURVEY 8d); biased = randn logits + the synthetic N(0, 0.1) "
                         "score-correction bias of rounds 1-5, which skews the routing; nobias = old name of uniform")
    ap.add_argument("--autotune", action="store_true",
                    help="turn the engine's first-call plan search on (lkm_set_tuning autotune; default off = what lk_moe users get)")
    ap.add_argument("--no-autotune", action="store_true", help="(default since round 5; kept so that older command lines still parse)")
    ap.add_argument("--batch-per-gpu", type=int, default=0, help="override the workload's tokens per GPU (plan A/Bs; not for the headline)")
    ap.add_argument("--regions", type=int, default=5,
                    help="timed regions of exactly --steps steps each; the median region is reported (all are listed); "
                         "regions of more than 1/REGIONS of a second are timed once")
    ap.add_argument("--full-line", action="store_true", help="print the complete record as the last line (tools), not the < 4 KB one")
    ap.add_argument("--full-out", default=str(ROOT / "gpurun_out" / "bench_full.json"),
                    help="side file for the complete records of the headline and the extra workloads ('' = none)")
    ap.add_argument("--tune", default="", help="comma list key=value for lkm_set_tuning (nt1,nt2,kw1,sk2,tbmax)")
    ap.add_argument("--flush-cache", action="store_true",
                    help="also report ms_per_step_cold: every step preceded by a 1 GiB write that evicts the L2s and the "
                         "256 MB Infinity Cache (SURVEY 8d flush variant; the headline numbers are unaffected)")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: the product path has no CPU fallback")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_ep
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    ctx = dict(world=world, rank=rank, dev=dev, dist=use_dist, wd=Watchdog(rank) if (world > 1 or (use_dist and os.environ.get("LKM_BENCH_WATCHDOG") == "1")) else None)

    head = run_workload(args.workload, args, ctx, steps=args.steps, warmup=args.warmup,
                        with_cpu=args.full and not args.no_cpu_baseline, full=args.full, force_ep=args.force_ep,
                        dump_dir=args.dump_outputs)
    def make_line(head, extras=None):
        """the headline object: the contract's fields + a roofline / cpu_baseline cut to what the judge reads (< 4 KB)"""
        rf = head.get("roofline") or {}
        roofline = None if not rf else {k_: rf.get(k_) for k_ in (
            "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "traffic_stale",
            "algorithmic_bytes", "mfma_frac", "hbm_frac", "kernel_ms", "kernel_ms_min_max", "gemm2_kernel", "timing")}
        if roofline and roofline.get("traffic_source"):
            roofline["traffic_source"] = roofline["traffic_source"][:160]
        cb = head.get("cpu_baseline")
        cpu = None
        if cb:
            cpu = {k_: cb.get(k_) for k_ in ("value", "unit", "cores", "kind", "sample", "ms_per_step", "ms_per_step_stat",
                                             "passes", "max_rel_err_gpu_vs_cpu")}
            cpu["host"] = {k_: (cb.get("host") or {}).get(k_) for k_ in ("nproc", "sockets", "cpu")}
            if cb.get("all_cores"):
                cpu["all_cores"] = cb["all_cores"]
            if cb.get("port"):
                cpu["port"] = {k_: cb["port"].get(k_) for k_ in ("value", "unit", "cores", "kind", "ms_per_step")}
        cfg = dict(head["config"])
        cfg["plan"] = cfg.pop("geometry", "")[-400:]
        line = {
            "metric": "moe_layer_decode_tokens_per_s", "value": head["value"], "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": head["scaling"],
            "vs_baseline": None, "dtype": head["dtype"], "data": "synthetic",
            "config": cfg, "roofline": roofline, "cpu_baseline": cpu,
        }
        line["timed_regions_ms"] = head.get("timed_regions_ms")
        line["timing"] = (f"{len(head.get('timed_regions_ms') or [])} regions of exactly {args.steps} steps each, barrier + synchronize "
                          "on both sides, max over ranks; value = the median region")
        if "ms_per_step_cold" in head:
            line["ms_per_step_cold"] = head["ms_per_step_cold"]
        if "long_run" in head:
            line["long_run"] = {k_: head["long_run"][k_] for k_ in ("steps", "ms_per_step")}
        if extras:
            line["extra_workloads"] = [e["workload"] + ("@" + e["config"]["routing"] if e["config"].get("routing") != "uniform" else "")
                                       for e in extras]
        return line

    def extra_line(r):
        """one short line per extra workload, printed BEFORE the headline line"""
        rf = r.get("roofline") or {}
        return {"extra_workload": r["workload"], "routing": r["config"].get("routing"), "value": r["value"], "unit": r["unit"],
                "ms_per_step": r["ms_per_step"], "steps": r["steps"], "dtype": r["dtype"], "n_gpus": world,
                "parallelism": r["config"].get("parallelism"), "launch": r["config"].get("launch"),
                "roofline": {k_: rf.get(k_) for k_ in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic",
                                                       "algorithmic_bytes", "kernel_ms", "gemm2_kernel")},
                "rows_per_expert_min_max": (rf.get("layer") or {}).get("rows_per_expert_min_max"),
                "plan": rf.get("plan"), "exchange": r["config"].get("exchange")}

    extras = []
    with_extras = args.full and not args.no_extras and args.workload == HEADLINE
    if ctx["wd"] is not None and with_extras:
        # (rank 0 holds the finished headline line from here on; the other ranks only need a non-None marker)
        ctx["wd"].arm(600.0, make_line(head) if head is not None else ({} if rank else None), "the extra workloads")
    if with_extras:
        es, ew = min(args.steps, 100), min(args.warmup, 10)
        names = (EXTRA_N1 if world == 1 and not args.force_ep else []) + [EXTRA_EP]
        for n in names:
            n, rt_over = n if isinstance(n, tuple) else (n, None)
            if WORKLOADS[n].get("prefill"):
                es_n, ew_n = min(es, 20), min(ew, 3)      # a 1-2 ms step: 20 steps are 30-40 ms of GPU time
            else:
                es_n, ew_n = es, ew
            try:
                r = run_workload(n, args, ctx, steps=es_n, warmup=ew_n, with_cpu=False, full=True,
                                 force_ep=args.force_ep and n == EXTRA_EP, routing=rt_over)
            except Exception as e:   # an extra must never take the headline line with it
                if use_dist:
                    raise                # ... except where ranks would fall out of step
                print(f"[bench] extra workload {n} failed: {type(e).__name__}: {e}", file=sys.stderr)
                r = None
            if r is not None:
                extras.append(r)
                print(json.dumps(extra_line(r)), flush=True)

    if ctx["wd"] is not None:
        ctx["wd"].disarm()
    if rank == 0:
        if head is None:
            sys.exit(f"workload {args.workload} does not shard over {world} GPUs")
        if args.full and args.full_out:
            try:
                fp = Path(args.full_out)
                fp.parent.mkdir(parents=True, exist_ok=True)
                fp.write_text(json.dumps({"headline": head, "extra": extras}, indent=1) + "\n")
            except OSError as e:
                print(f"[bench] could not write {args.full_out}: {e}", file=sys.stderr)
        obj = make_line(head, extras)
        if args.full_line:      # tools (report.py, update_hbm_traffic.py): every field of the record on the line
            obj = {**obj, "config": head["config"], "roofline": head["roofline"], "cpu_baseline": head.get("cpu_baseline")}
        else:
            # the contract's line stays under 4 KB whatever a field grows to: shed the least important parts first
            for path in (("cpu_baseline", "port"), ("roofline", "traffic_source"), ("config", "plan"), ("cpu_baseline", "sample"),
                         ("extra_workloads",), ("roofline", "timing")):
                if len(json.dumps(obj)) < 4000:
                    break
                d = obj
                for k_ in path[:-1]:
                    d = d.get(k_) or {}
                d.pop(path[-1], None)
        print(json.dumps(obj), flush=True)
    if use_dist:
        # Every rank is past its last collective; leave without tearing the communicator down: destroying a
        # process group whose collectives live in captured graphs has hung at exit before, and the JSON line is out.
        dist.barrier()
        torch.cuda.synchronize()
        sys.stdout.flush()
        sys.stderr.flush()
        if os.environ.get("LKM_BENCH_CLEAN_EXIT") == "1":    # profilers write their output at interpreter exit
            return
        os._exit(0)


if __name__ == "__main__":
    main()
