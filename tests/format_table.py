"""One entry per engine configuration: seeded weights, the engine built from them and the CPU reference of the same layer, with
the tolerance that the format's own test file uses.  A plain helper module (tests/test_gpu_call_paths.py and
tests/test_format_table.py import it); the builders, references and tolerances are the ones of the format's test file, imported
from there.

    case = FORMATS[name].make(E, H, I, K, gated, dt, seed)     # CPU only: weights and reference
    eng = case.engine(**engine_kw)                             # needs the GPU
    ref = case.ref(a, ids, tw)                                 # float64 [M, H] from the inputs alone (a: CPU tensor of the activation dtype)
    case.check(out, ref, what, rounded=False)                  # rounded: `out` was written in the activation dtype
    FORMATS[name].build(E, H, I, K, gated, dt, seed, **engine_kw) -> (eng, ref)

Non-gated layers are relu2 (activation_type 2), gated ones SiLU.  Shape families: A for every entry, B (K loops that are no whole
128 / 256 units) where the format admits it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from lvllm_amd import _clib
from oracle import oracle as orc
from tests import test_gpu_int4_zp as t_zp
from tests import test_gpu_int8_a8 as t_i8a
from tests import test_gpu_int8_native as t_i8
from tests import test_gpu_moe as t_moe
from tests import test_gpu_mxfp4_a4 as t_a4
from tests import test_gpu_mxfp4_a8 as t_a8
from tests.helpers import bits_to_torch, make_routing, torch_to_bits

FAMILY_A = dict(E=8, K=2, H=256, I=128)
FAMILY_B = dict(E=4, K=2, H=160, I=96)
ATOL, RTOL = t_moe.ATOL, t_moe.RTOL


def rnd(x, tdt):                                   # float64 -> the activation dtype (RNE) -> float64
    return t_a8.rnd(x, tdt)


@dataclass
class Case:
    name: str
    E: int
    H: int
    I: int
    K: int
    gated: bool
    dt: torch.dtype
    engine: Callable          # (**engine_kw) -> RoutedExpertsEngine
    ref: Callable             # (a, ids, tw) -> float64 [M, H]
    tol: Callable             # (out, ref, what, rounded) -> None, raises

    def check(self, out, ref, what="", rounded=False):
        out = np.asarray(out, np.float64)
        ref = rnd(ref, self.dt) if rounded else np.asarray(ref, np.float64)
        err = np.abs(out - ref)
        print(f"{self.name} {what}: max|ref|={np.abs(ref).max():.4g} max err={err.max():.4g}")
        self.tol(out, ref, f"{self.name} {what}", rounded)


@dataclass
class Format:
    name: str
    make: Callable            # (E, H, I, K, gated, dt, seed) -> Case
    dt: torch.dtype = torch.bfloat16
    family_b: bool = False    # admits H = 160, I = 96
    exact_sums: bool = False  # every plan gives the same sums: plans compare at 1e-5 of the scale (the format's test_plans_agree)
    relu2_images: bool = False

    def build(self, E, H, I, K, gated, dt, seed, **engine_kw):
        case = self.make(E, H, I, K, gated, dt, seed)
        return case.engine(**engine_kw), case.ref


def _odt(dt):
    return orc.BF16 if dt == torch.bfloat16 else orc.F16


def _gkw(gated):                                   # engine / oracle keywords of a non-gated relu2 layer
    return ({}, {}) if gated else (dict(has_gate_proj=False, activation_type=2), dict(has_gate=False, activation=orc.ACT_RELU2))


def _master(E, H, I, gated, dt, seed):             # 16-bit master weights, randn / 10 (tests/test_gpu_moe.py::_rand_case)
    _, w13, w2, _, _ = t_moe._rand_case(1, E, 1, H, I, dt, seed, gated=gated)
    return w13, w2


def _tol_abs(atol, rtol):                          # the oracle tolerance of tests/test_gpu_moe.py
    def tol(out, ref, what, rounded):
        np.testing.assert_allclose(out, ref, atol=atol, rtol=rtol, err_msg=what)
    return tol


def _tol_scaled(atol, rtol, atol_r=None, rtol_r=None, floor=0.0):
    """atol times the output scale (max|ref|, at least `floor`); atol_r / rtol_r: the format's figures for activation-dtype output"""
    def tol(out, ref, what, rounded):
        scale = max(floor, float(np.abs(ref).max()))
        a, r = (atol_r, rtol_r) if rounded and atol_r is not None else (atol, rtol)
        np.testing.assert_allclose(out, ref, atol=a * scale, rtol=r, err_msg=what)
    return tol


def _orc_ref(desc, w13, w2, dt, **okw):
    def ref(a, ids, tw):
        return orc.moe(desc, w13, w2, torch_to_bits(a), np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(tw, np.float32), **okw).astype(np.float64)
    return ref


def _make_16bit(name):
    def make(E, H, I, K, gated, dt, seed):
        w13, w2 = _master(E, H, I, gated, dt, seed)
        ekw, okw = _gkw(gated)
        d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=_odt(dt), wfmt=orc.W_BF16 if dt == torch.bfloat16 else orc.W_F16, **okw)
        eng = lambda **kw: t_moe._eng(w13, w2, top_k=K, act_dtype=dt, fmt="bf16" if dt == torch.bfloat16 else "fp16", **ekw, **kw)
        return Case(name, E, H, I, K, gated, dt, eng, _orc_ref(d, torch_to_bits(w13), torch_to_bits(w2), dt), _tol_abs(ATOL, RTOL))
    return make


def _make_int4(name, fast):
    g = 128 if fast else 64

    def make(E, H, I, K, gated, dt, seed):
        w13, w2 = _master(E, H, I, gated, dt, seed)
        odt = _odt(dt)
        ekw, okw = _gkw(gated)
        q13, s13 = orc.quant_int4(torch_to_bits(w13), odt, g)
        q2, s2 = orc.quant_int4(torch_to_bits(w2), odt, g)
        d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=odt, wfmt=orc.W_INT4, groupN=1, groupK=g, int4_unrounded=fast, **okw)
        mode = dict(int4_mode=_clib.INT4_FAST) if fast else {}
        eng = lambda **kw: t_moe._eng(torch.from_numpy(q13), torch.from_numpy(q2), top_k=K, act_dtype=dt, fmt="int4", w13_scale=bits_to_torch(s13, odt),
                                      w2_scale=bits_to_torch(s2, odt), group_n=1, group_k=g, **mode, **ekw, **kw)
        # fast mode: test_int4_fast_mode_golden_cases_and_random_shapes scales atol by max|ref|
        return Case(name, E, H, I, K, gated, dt, eng, _orc_ref(d, q13, q2, dt, s13=s13, s2=s2), _tol_scaled(ATOL, RTOL) if fast else _tol_abs(ATOL, RTOL))
    return make


def _make_wna16(name, bits, zp):
    """int4 with zero points (g = 64) and native 8-bit with / without them (g = 128): the weights of the formats' `_case`, dequantised
    by orc.dequant_wna16 and run through orc.moe as 16-bit weights (test_zero_point_layers_vs_oracle / test_int8_layers_vs_oracle)"""
    g = 64 if bits == 4 else 128

    def make(E, H, I, K, gated, dt, seed):
        odt = _odt(dt)
        ekw, okw = _gkw(gated)
        rng = np.random.default_rng(seed)
        n13 = (2 if gated else 1) * I
        if bits == 4:
            q13, s13, z13 = t_zp._case(rng, E, n13, H, g, odt, wide=False)
            q2, s2, z2 = t_zp._case(rng, E, H, I, g, odt, wide=False)
            d13, d2 = orc.dequant_wna16(q13, s13, t_zp._pack_zp(z13), 4, g, odt), orc.dequant_wna16(q2, s2, t_zp._pack_zp(z2), 4, g, odt)
            eng = lambda **kw: t_zp._eng(torch.from_numpy(q13), torch.from_numpy(q2), top_k=K, act_dtype=dt, fmt="int4", w13_scale=bits_to_torch(s13, odt),
                                         w2_scale=bits_to_torch(s2, odt), group_n=1, group_k=g, w13_zp=torch.from_numpy(z13), w2_zp=torch.from_numpy(z2), **ekw, **kw)
        else:
            q13, s13, z13 = t_i8._case(rng, E, n13, H, g, odt, zp)
            q2, s2, z2 = t_i8._case(rng, E, H, I, g, odt, zp)
            d13, d2 = orc.dequant_wna16(q13, s13, z13, 8, g, odt), orc.dequant_wna16(q2, s2, z2, 8, g, odt)
            eng = lambda **kw: t_i8._eng(q13, q2, s13, s2, z13, z2, odt, group_k=g, top_k=K, act_dtype=dt, **ekw, **kw)
        d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=odt, wfmt=orc.W_BF16 if dt == torch.bfloat16 else orc.W_F16, **okw)
        return Case(name, E, H, I, K, gated, dt, eng, _orc_ref(d, d13, d2, dt), _tol_scaled(2e-3, 1e-2, 4e-3, 1.5e-2))
    return make


def _make_int8a8(E, H, I, K, gated, dt, seed):
    w = t_i8a.make_weights(np.random.default_rng(seed), E, H, I, gated)
    act = "silu" if gated else "relu2"
    ref = lambda a, ids, tw: t_i8a.ref_layer(a.to(torch.float64).numpy(), *w, ids, np.asarray(tw, np.float64), act, dt)
    return Case("int8a8", E, H, I, K, gated, dt, lambda **kw: t_i8a.engine(*w, dt, K, act, **kw), ref, lambda o, r, what, rounded: t_i8a.check(o, r, what))


def _make_fp8(name, a8):
    def make(E, H, I, K, gated, dt, seed):
        w13, w2 = _master(E, H, I, gated, dt, seed)
        ekw, okw = _gkw(gated)
        q13, s13 = orc.quant_fp8_block(w13.float().numpy(), 128, 128)
        q2, s2 = orc.quant_fp8_block(w2.float().numpy(), 128, 128)
        d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=_odt(dt), wfmt=orc.W_FP8, groupN=128, groupK=128, round_gemm1=a8, w8a8=a8, **okw)
        eng = lambda **kw: t_moe._eng(torch.from_numpy(q13), torch.from_numpy(q2), top_k=K, act_dtype=dt, fmt="fp8", w13_scale=torch.from_numpy(s13),
                                      w2_scale=torch.from_numpy(s2), group_n=128, group_k=128, fp8_mode=_clib.FP8_W8A8 if a8 else _clib.FP8_W8A16, **ekw, **kw)
        # test_fp8_w8a16_golden_inputs / test_fp8_w8a8_block_golden_and_oracle
        return Case(name, E, H, I, K, gated, dt, eng, _orc_ref(d, q13, q2, dt, s13=s13, s2=s2), _tol_scaled(1e-2, 2e-2) if a8 else _tol_abs(ATOL, RTOL))
    return make


def _make_fp4(name):
    """weight-only MXFP4 / NVFP4: random E2M1 codes and scale bytes, NVFP4 with per-expert multipliers (the inputs of
    tests/test_gpu_moe.py::test_prefill_kernel_4bit_formats), tolerance of test_fp4_golden_cases"""
    def make(E, H, I, K, gated, dt, seed):
        ekw, okw = _gkw(gated)
        rng = np.random.default_rng(seed)
        n13 = (2 if gated else 1) * I
        g, wf, lo, hi = (32, orc.W_MXFP4, 117, 121) if name == "mxfp4" else (16, orc.W_NVFP4, 0x18, 0x28)
        q13, q2 = rng.integers(0, 256, (E, n13, H // 2), dtype=np.uint8), rng.integers(0, 256, (E, H, I // 2), dtype=np.uint8)
        s13, s2 = rng.integers(lo, hi, (E, n13, H // g), dtype=np.uint8), rng.integers(lo, hi, (E, H, I // g), dtype=np.uint8)
        gkw, gokw = {}, {}
        if name == "nvfp4":
            gs13, gs2 = rng.uniform(0.5, 2.0, E).astype(np.float32), rng.uniform(0.5, 2.0, E).astype(np.float32)
            gkw, gokw = dict(w13_global_scale=torch.from_numpy(gs13), w2_global_scale=torch.from_numpy(gs2)), dict(gs13=gs13, gs2=gs2)
        d = orc.MoeDesc(E=E, H=H, I=I, act_dtype=_odt(dt), wfmt=wf, groupN=1, groupK=g, **okw)
        eng = lambda **kw: t_moe._eng(torch.from_numpy(q13), torch.from_numpy(q2), top_k=K, act_dtype=dt, fmt=name, w13_scale=torch.from_numpy(s13),
                                      w2_scale=torch.from_numpy(s2), group_n=1, group_k=g, **gkw, **ekw, **kw)
        return Case(name, E, H, I, K, gated, dt, eng, _orc_ref(d, q13, q2, dt, s13=s13, s2=s2, **gokw), _tol_scaled(ATOL, RTOL, floor=1.0))
    return make


def _make_mxa(name, mod):
    def make(E, H, I, K, gated, dt, seed):
        q13, q2, s13, s2 = mod.make_weights(np.random.default_rng(seed), E, H, I, gated)
        w13, w2 = mod.deq_w(q13, s13), mod.deq_w(q2, s2)
        act = "silu" if gated else "relu2"
        ref = lambda a, ids, tw: mod.ref_layer(a.to(torch.float64).numpy(), w13, w2, ids, np.asarray(tw, np.float64), act, dt)
        return Case(name, E, H, I, K, gated, dt, lambda **kw: mod.engine(q13, q2, s13, s2, dt, K, act, **kw), ref,
                    lambda o, r, what, rounded: mod.check(o, r, what))
    return make


FORMATS = {f.name: f for f in [
    Format("bf16", _make_16bit("bf16"), family_b=True, relu2_images=True),
    Format("f16", _make_16bit("f16"), dt=torch.float16),
    Format("int4", _make_int4("int4", False)),
    Format("int4fast", _make_int4("int4fast", True)),
    Format("int4zp", _make_wna16("int4zp", 4, True)),
    Format("int8", _make_wna16("int8", 8, False)),
    Format("int8zp", _make_wna16("int8zp", 8, True)),
    Format("int8a8", _make_int8a8, family_b=True, exact_sums=True, relu2_images=True),
    Format("fp8", _make_fp8("fp8", False)),
    Format("fp8a8", _make_fp8("fp8a8", True)),
    Format("mxfp4", _make_fp4("mxfp4")),
    Format("nvfp4", _make_fp4("nvfp4")),
    Format("mxfp4a8", _make_mxa("mxfp4a8", t_a8), family_b=True, exact_sums=True, relu2_images=True),
    Format("mxfp4a4", _make_mxa("mxfp4a4", t_a4), family_b=True, exact_sums=True),
]}
NAMES = list(FORMATS)
# the modes with scratch of their own for quantised activations, scales or row sums (chunk_tokens limits each)
QUANTISED_ACTIVATIONS = ["int4fast", "fp8a8", "int8a8", "mxfp4a8", "mxfp4a4"]
# (name, family) pairs: A everywhere, B where the K loops may be ragged
SHAPED = [(n, "A") for n in NAMES] + [(n, "B") for n in NAMES if FORMATS[n].family_b]


def make_case(name, family="A", gated=True, seed=0):
    f = FORMATS[name]
    s = FAMILY_A if family == "A" else FAMILY_B
    return f.make(s["E"], s["H"], s["I"], s["K"], gated, f.dt, seed)


# ---------------------------------------------------------------------------------------------- inputs of the call-path cases
def hidden(M, H, dt, seed):                        # randn / 4, as the formats' whole-layer tests
    return (torch.randn((M, H), generator=torch.Generator().manual_seed(seed)) / 4).to(dt)


def routing(M, E, K, seed):
    """make_routing with 10 % dropped slots and one expert left empty -> (tw fp32 [M, K], ids int32 [M, K])"""
    tw, ids = make_routing(M, E, K, seed=seed, drop=0.1)
    ids[ids == E - 1] = -1
    return tw, ids


def window_case(M, K, seed, router_experts=16, first=4, local=8):
    """global ids over `router_experts` experts for an engine that holds [first, first + local) -> (tw, global ids, local ids with
    -1 outside the window)"""
    tw, gids = make_routing(M, router_experts, K, seed=seed, drop=0.1)
    inside = (gids >= first) & (gids < first + local)
    return tw, gids, np.where(inside, gids - first, -1).astype(np.int32)


def window_case_is_complete(gids, lids, first=4, local=8):
    """the conditions the local-window test states: ids below, inside and above the window, a token without any local expert"""
    below, above = (gids >= 0) & (gids < first), gids >= first + local
    return bool(below.any() and above.any() and (lids >= 0).any() and (lids < 0).all(axis=1).any())


def strided_inputs(a, tw, ids, E, poison, pad_h=24, pad_k=3, lead_h=8, lead_k=1):
    """the clean rows as views into wider, poisoned matrices: hidden in [M, H + pad_h] (columns lead_h ..), ids and weights in
    [M, K + pad_k] (columns lead_k ..).  Gaps: `poison` in the hidden rows, E + 7 in the ids, 1e30 in the weights."""
    M, H = a.shape
    K = ids.shape[1]
    big_a = torch.full((M, H + pad_h), poison, dtype=a.dtype)
    big_i = torch.full((M, K + pad_k), E + 7, dtype=torch.int32)
    big_w = torch.full((M, K + pad_k), 1e30, dtype=torch.float32)
    big_a[:, lead_h:lead_h + H] = a
    big_i[:, lead_k:lead_k + K] = torch.from_numpy(ids)
    big_w[:, lead_k:lead_k + K] = torch.from_numpy(tw)
    view = lambda t, lead, n: t[:, lead:lead + n]
    return (big_a, big_w, big_i), lambda ta, tw_, ti: (view(ta, lead_h, H), view(tw_, lead_k, K), view(ti, lead_k, K))
