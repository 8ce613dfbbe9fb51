"""Weight-only 8-bit experts (uint8b128 / uint8 + zero points) on the native one-byte format (LKM_W_INT8, include/lkm.h) against
the oracle's dequant_wna16: bit for bit through one-hot activations on every path, whole layers, the modular surface."""
import types

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.helpers import bits_to_torch, make_routing, torch_to_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = {"bf16": (orc.BF16, torch.bfloat16, "bf16"), "f16": (orc.F16, torch.float16, "fp16")}


def _eng(q13, q2, s13b, s2b, z13, z2, odt, **k):
    from lvllm_amd.ops import RoutedExpertsEngine
    t = lambda z: None if z is None else torch.from_numpy(z)
    return RoutedExpertsEngine(torch.from_numpy(q13), torch.from_numpy(q2), fmt="int8", w13_scale=bits_to_torch(s13b, odt),
                               w2_scale=bits_to_torch(s2b, odt), group_n=1, w13_zp=t(z13), w2_zp=t(z2), **k)


def _case(rng, E, N, K, g, odt, zp, lo=5e-4, hi=4e-3):      # layers: |w| <= 255 * 4e-3 ~ 1, finite in fp16
    q = rng.integers(0, 256, (E, N, K), dtype=np.uint8)
    s = orc.f32_to_bits(rng.uniform(lo, hi, (E, N, K // g)).astype(np.float32), odt)
    return q, s, (rng.integers(0, 256, (E, N, K // g), dtype=np.uint8) if zp else None)


@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("g", [32, 64, 128, 256])
def test_int8_dequant_is_bit_exact(g, dt, zp):
    E, H, I = 2, 256, 128
    odt, tdt, _ = DTS[dt]
    rng = np.random.default_rng(83 + g)
    q13, s13b, z13 = _case(rng, E, I, H, g, odt, zp, 0.002, 0.2)          # two decades; 255 * 0.2 is finite in fp16
    for j in range(H // g):                                               # the edge codes in every group of row 0 of expert 0 ...
        q13[0, 0, j * g: j * g + 7] = [0, 1, 127, 128, 129, 254, 255]
    if zp:
        z13[0, 0, :] = np.array([0, 255, 128, 1, 254, 0, 255, 128], np.uint8)[: H // g]      # ... against the edge zero points
    wd = orc.bits_to_f32(orc.dequant_wna16(q13, s13b, z13, 8, g, odt), odt)                   # [E, I, H]
    q2 = np.full((E, H, I), 128, np.uint8)                                # w2 = identity: (128 - 128) * 1 = 0 ...
    q2[:, np.arange(I), np.arange(I)] = 129                               # ... and (129 - 128) * 1 = 1 on the diagonal
    s2b = orc.f32_to_bits(np.ones((E, H, I // min(g, I)), np.float32), odt)
    eng = _eng(q13, q2, s13b, s2b, z13, np.full((E, H, I // min(g, I)), 128, np.uint8) if zp else None, odt, top_k=1, act_dtype=tdt,
               group_k=g, has_gate_proj=False, activation_type=2)
    assert "wf=6" in eng.engine.describe()
    tw = torch.ones((H, 1), dtype=torch.float32, device=DEV)
    for e in range(E):
        ids = torch.full((H, 1), e, dtype=torch.int32, device=DEV)
        for tiled in (0, -1, 32, 64, 128):     # the planner's own choice, the forced streamer, every height of the tile kernel
            eng.engine.set_tuning(pf=-1 if tiled > 0 else 0, tiled=tiled)
            for sign in (1.0, -1.0):
                out = eng.decode((torch.eye(H) * sign).to(tdt).to(DEV), tw, ids).cpu().numpy()[:, :I]
                want = (np.maximum(sign * wd[e].T, 0.0) ** 2).astype(np.float32)              # out[j, i] = T(relu(+-W[e, i, j])^2)
                np.testing.assert_array_equal(out, orc.bits_to_f32(orc.f32_to_bits(want, odt), odt),
                                              err_msg=f"g={g} e={e} tiled={tiled} sign={sign} {eng.engine.describe()}")


@pytest.mark.parametrize("M,E,K,H,I,g,dt,gated,zp,prefill", [
    (1, 8, 2, 512, 256, 128, "bf16", True, False, False),      # one token: the streamer
    (32, 8, 2, 512, 384, 128, "bf16", True, False, False),     # decode batch
    (128, 8, 2, 512, 384, 64, "f16", True, True, False),       # two groups per unit, tile kernel
    (77, 4, 2, 256, 128, 32, "bf16", True, True, False),       # ragged, four groups per unit
    (33, 16, 4, 256, 128, 128, "bf16", False, False, False),   # relu2, non-gated
    (600, 4, 2, 256, 256, 256, "bf16", True, False, True),     # prefill-sized, one group per two units
    (2000, 6, 2, 384, 256, 128, "f16", True, True, True),      # ~670 rows per expert (128-row tiles: the format has no 256-row kernel)
])
def test_int8_layers_vs_oracle(M, E, K, H, I, g, dt, gated, zp, prefill):
    from lvllm_amd.ops import RoutedExpertsEngine
    odt, tdt, f16 = DTS[dt]
    rng = np.random.default_rng(11 + M)
    q13, s13b, z13 = _case(rng, E, (2 if gated else 1) * I, H, g, odt, zp)
    q2, s2b, z2 = _case(rng, E, H, I, g, odt, zp)
    kw = dict(top_k=K, act_dtype=tdt, **({} if gated else dict(has_gate_proj=False, activation_type=2)))
    eng = _eng(q13, q2, s13b, s2b, z13, z2, odt, group_k=g, **kw)
    d13, d2 = orc.dequant_wna16(q13, s13b, z13, 8, g, odt), orc.dequant_wna16(q2, s2b, z2, 8, g, odt)
    desc = orc.MoeDesc(E=E, H=H, I=I, act_dtype=odt, wfmt=orc.W_BF16 if dt == "bf16" else orc.W_F16,
                       **({} if gated else dict(has_gate=False, activation=orc.ACT_RELU2)))
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) / 10).to(tdt)
    tw, ids = make_routing(M, E, K, seed=M, drop=0.05)
    ref = orc.moe(desc, d13, d2, torch_to_bits(a), ids, tw)
    scale = float(np.abs(ref).max())
    assert np.isfinite(ref).all() and scale > 0
    twd, idd = torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    run = lambda en: (en.prefill(a.to(DEV), twd, idd).float() if prefill else en.decode(a.to(DEV), twd, idd)).cpu().numpy()
    out = run(eng)
    np.testing.assert_allclose(out, ref, atol=(4e-3 if prefill else 2e-3) * scale, rtol=1.5e-2 if prefill else 1e-2, err_msg=eng.engine.describe())
    # the 16-bit engine on the same dequantised operands: fp32 accumulation in another order
    e16 = RoutedExpertsEngine(bits_to_torch(d13, odt), bits_to_torch(d2, odt), fmt=f16, **kw)
    np.testing.assert_allclose(out, run(e16), atol=(4e-3 if prefill else 1e-3) * scale, rtol=1.5e-2 if prefill else 5e-3)


@pytest.mark.parametrize("zp", [False, True])
def test_int8_modular_surface(zp, monkeypatch):
    from lvllm_amd.modular import LkmExperts
    M, E, K, H, I, g = 24, 4, 2, 256, 128, 128
    rng = np.random.default_rng(5)
    q13, s13b, z13 = _case(rng, E, 2 * I, H, g, orc.BF16, zp)
    q2, s2b, z2 = _case(rng, E, H, I, g, orc.BF16, zp)
    dev = lambda z: None if z is None else torch.from_numpy(z).to(DEV)
    qc = types.SimpleNamespace(w1_scale=bits_to_torch(s13b, orc.BF16).to(DEV), w2_scale=bits_to_torch(s2b, orc.BF16).to(DEV),
                               block_shape=[0, g], use_int8_w8a16=True, w1_zp=dev(z13), w2_zp=dev(z2))
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(9)) / 10).to(torch.bfloat16)
    tw, ids = make_routing(M, E, K, seed=9)
    ref = orc.moe(orc.MoeDesc(E=E, H=H, I=I, act_dtype=orc.BF16), orc.dequant_wna16(q13, s13b, z13, 8, g, orc.BF16),
                  orc.dequant_wna16(q2, s2b, z2, 8, g, orc.BF16), torch_to_bits(a), ids, tw)
    held = {}
    for expand in ("0", "1"):       # "0" = nothing with a native format is expanded (8-bit: opt-in on this surface), "1" = everything is
        monkeypatch.setenv("LKM_WNA16_EXPAND", expand)
        ex = LkmExperts(None, qc)
        out = torch.empty((M, H), dtype=torch.bfloat16, device=DEV)
        ex.apply(out, a.to(DEV), dev(q13), dev(q2), dev(tw), dev(ids), "silu", E, None, None, None, None, None, None, False)
        assert ("wf=0" if expand == "1" else "wf=6") in ex._engine.engine.describe()
        np.testing.assert_allclose(out.float().cpu().numpy(), ref, atol=2e-3 * float(np.abs(ref).max()), rtol=1e-2)
        held[expand] = ex._engine.engine.weight_bytes()
    assert held["0"] <= 0.6 * held["1"], held                             # (1 + 4 / g) / 2 of the expansion, plus padding


def test_int8_arguments_are_checked():
    from lvllm_amd._clib import LkmError
    E, H, I, g = 2, 256, 128, 128
    rng = np.random.default_rng(3)
    q13, s13b, z13 = _case(rng, E, 2 * I, H, g, orc.BF16, True)
    q2, s2b, z2 = _case(rng, E, H, I, g, orc.BF16, True)
    # one zero-point tensor without the other; a zero-point tensor of the wrong shape; a group of 48
    for za, zb, gk, exc in ((z13, None, g, ValueError), (z13[:, :4], z2, g, ValueError), (None, None, 48, LkmError)):
        with pytest.raises(exc):
            _eng(q13, q2, s13b, s2b, za, zb, orc.BF16, group_k=gk, top_k=2, act_dtype=torch.bfloat16)
