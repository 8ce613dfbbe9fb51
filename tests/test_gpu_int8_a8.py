"""int8 weights x per-token int8 activations (LKM_W_INT8 with fp8_mode = LKM_FP8_W8A8: gemm_i8a8_kernel on the integer MFMA) against
a numpy restatement of the mode's numerics: quantiser bytes (float32, operation for operation), the operand layout on one tile,
whole layers (float64 on the same quantised operands), plan parity."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from lvllm_amd import _clib
from tests.helpers import make_routing

gpu = pytest.mark.gpu
DEV = "cuda:0"
ACTS = {"silu": dict(activation_type=0), "swigluoai": dict(activation_type=1), "relu2": dict(activation_type=2, has_gate_proj=False)}
F32 = np.float32


def rnd(x, tdt):                                   # float64 -> the activation dtype (RNE) -> float64
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(tdt).to(torch.float64).numpy()


def q8(x):
    """x [R, K] (16-bit values) -> (int8 [R, K], float32 scales [R]): amax / 127, rint(x * (127 / amax)) in float32, ties to even"""
    x = x.astype(F32)
    amax = np.abs(x).max(-1)
    with np.errstate(divide="ignore"):
        inv = np.where(amax == 0, F32(0), F32(127) / amax).astype(F32)
    return np.clip(np.rint(x * inv[:, None]), -128, 127).astype(np.int8), (amax / F32(127)).astype(F32)


def act_fn(g1, act, tdt):                          # the rounded GEMM1 output -> the intermediate, rounded (ref_layer's two rounding points)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    if act == "silu":
        I = g1.shape[1] // 2
        return rnd(rnd(g1[:, :I] * sig(g1[:, :I]), tdt) * g1[:, I:], tdt)
    if act == "swigluoai":
        g, u = np.minimum(g1[:, 0::2], 7.0), np.clip(g1[:, 1::2], -7.0, 7.0)
        return rnd((u + 1.0) * g * sig(g * 1.702), tdt)
    return rnd(np.maximum(g1, 0.0) ** 2, tdt)


def ref_layer(a, w13, s13, w2, s2, ids, tw, act, tdt):
    """the specification: per-token int8 tokens, exact integer GEMM1 times both scales rounded to tdt, activation on the rounded
    value, rounded, per-token int8 along I, GEMM2, router weights"""
    xq, xs = q8(a)
    out = np.zeros((a.shape[0], w2.shape[1]))
    for e in range(w13.shape[0]):
        m, k = np.nonzero(ids == e)
        if not len(m):
            continue
        g1 = rnd((xq[m].astype(np.float64) @ w13[e].T.astype(np.float64)) * xs[m, None] * s13[e][None, :], tdt)
        hq, hs = q8(act_fn(g1, act, tdt))
        np.add.at(out, m, tw[m, k][:, None] * ((hq.astype(np.float64) @ w2[e].T.astype(np.float64)) * hs[:, None] * s2[e][None, :]))
    return out


def engine(w13, s13, w2, s2, tdt, K, act="silu", fp8_mode=_clib.FP8_W8A8, **kw):
    from lvllm_amd.ops import RoutedExpertsEngine
    big = max(w13.shape[2], w2.shape[2])
    t = torch.from_numpy
    return RoutedExpertsEngine(t(w13), t(w2), fmt="int8", w13_scale=t(s13), w2_scale=t(s2), group_n=1, group_k=kw.pop("group_k", big), top_k=K,
                               act_dtype=tdt, fp8_mode=fp8_mode, **ACTS[act], **kw)


def make_weights(rng, E, H, I, gated):             # uniform over [-128, 127] (-128 included), scales rand * 1e-2 (test_int8_kernel.py)
    n13 = (2 if gated else 1) * I
    return (rng.integers(-128, 128, (E, n13, H), dtype=np.int8), (rng.random((E, n13), dtype=F32) * F32(1e-2)),
            rng.integers(-128, 128, (E, H, I), dtype=np.int8), (rng.random((E, H), dtype=F32) * F32(1e-2)))


def check(out, ref, what=""):                     # the W8A8 tolerance of tests/test_gpu_moe.py, every element
    err = np.abs(out - ref)
    print(f"{what} max|ref|={np.abs(ref).max():.4g} max err={err.max():.4g} differing={int((err > 0).sum())}/{err.size}")
    np.testing.assert_allclose(out, ref, atol=1e-2 * np.abs(ref).max(), rtol=2e-2, err_msg=what)


@gpu
@pytest.mark.parametrize("rows,cols,ld", [(1, 32, 32), (5, 160, 168), (33, 4096, 4096)])
@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16])
def test_quantiser_bytes_and_scales_exact(tdt, rows, cols, ld):
    from lvllm_amd import ops
    x = torch.randn((rows, ld), generator=torch.Generator().manual_seed(cols)).to(tdt)
    ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -3.5]).repeat(cols // 8)       # -> 0 -0 2 -2 2 -2 126 -4 at scale 1
    ties[9] = 127.0
    top = torch.rand(cols, generator=torch.Generator().manual_seed(1)) * 0.4 * torch.finfo(tdt).max
    top[3] = -torch.finfo(tdt).max
    planted = [torch.zeros(cols), ties, top]
    if tdt == torch.float16:
        planted.append(torch.randint(-1023, 1024, (cols,), generator=torch.Generator().manual_seed(2)) * 2.0 ** -24)   # subnormals only
    for i, row in enumerate(planted):              # (the single row of the first shape holds only the last of them)
        x[i % rows, :cols] = row.to(tdt)
    xd = x.to(DEV)[:, :cols]                        # sliced on the device: the rows keep their stride ld
    assert xd.stride(0) == ld
    q, s = ops.quant_int8_rows(xd)
    rq, rs = q8(xd.cpu().to(torch.float32).numpy())
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    np.testing.assert_array_equal(q.cpu().numpy(), rq)
    if rows > 1:
        assert rs[0] == 0 and not rq[0].any() and rs[1] == 1 and list(rq[1, :8]) == [0, 0, 2, -2, 2, -2, 126, -4]


@gpu
@pytest.mark.parametrize("M", [1, 16])
def test_one_tile_pins_operand_layout(M):
    H, I, tdt = 128, 32, torch.bfloat16
    n, k = np.arange(2 * I)[:, None], np.arange(H)[None, :]
    w13 = (((n * 37 + (k // 16) * 11 + k * 3) % 255) - 127).astype(np.int8)[None]      # every row and every 16-k piece distinct
    s13 = ((1 + np.arange(2 * I)) * 1e-3).astype(F32)[None]                            # ... and a scale per row
    w2 = np.zeros((1, H, I), np.int8)                                                  # w2: 1 at column h % I of output row h, scale 1
    w2[0, np.arange(H), np.arange(H) % I] = 1
    s2 = np.ones((1, H), F32)
    eng = engine(w13, s13, w2, s2, tdt, 1)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) * torch.linspace(0.05, 2.0, H)).to(tdt)
    ids, tw = np.zeros((M, 1), np.int32), np.ones((M, 1), np.float32)
    out = eng.decode(a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)).cpu().numpy()
    check(out, ref_layer(a.to(torch.float64).numpy(), w13, s13, w2, s2, ids, tw, "silu", tdt), eng.engine.describe())


# the shapes of tests/test_gpu_mxfp4_a8.py: across a 128-row tile, an empty expert, K loops that are not whole units (160, 96, 1184, 1056)
SHAPES = [(1, 4, 2, 160, 96), (17, 4, 2, 160, 96), (130, 2, 1, 256, 128), (70, 8, 2, 512, 384), (33, 4, 2, 1184, 1056)]


@gpu
@pytest.mark.parametrize("M,E,K,H,I,act,tdt", [(*s, act, torch.bfloat16) for s in SHAPES for act in ACTS] +
                         [(*SHAPES[1], "silu", torch.float16)])
def test_whole_layer(M, E, K, H, I, act, tdt):
    w = make_weights(np.random.default_rng(M + H), E, H, I, act != "relu2")
    eng = engine(*w, tdt, K, act)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) / 4).to(tdt)
    tw, ids = make_routing(M, E, K, seed=M, drop=0.1)
    ids[ids == E - 1] = -1                                                        # one expert stays empty
    if M == 130:
        ids[:] = 0                                                                # every token on expert 0: 130 rows cross the 128-row tile
    ref = ref_layer(a.to(torch.float64).numpy(), *w, ids, tw.astype(np.float64), act, tdt)
    ad, twd, idd = a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    check(eng.decode(ad, twd, idd).cpu().numpy(), ref, "decode " + eng.engine.describe())
    assert all("gemm_i8a8_kernel" in k for g in ("gemm1", "gemm2") for k in eng.engine.last_kernels()[g]), eng.engine.last_kernels()
    check(eng.prefill(ad, twd, idd).float().cpu().numpy(), rnd(ref, tdt), "gpu_prefill")


def w8a16_case():
    """inputs on which integer activations show: one element per row ~100 x the rest sets the token's scale, so per-token int8 zeroes
    most of the row; its weight column is 0, so what is lost is the layer's whole signal.  -> the two float64 references"""
    M, E, K, H, I, tdt = 17, 4, 2, 256, 128, torch.bfloat16
    w13, s13, w2, s2 = make_weights(np.random.default_rng(9), E, H, I, True)
    w13[:, :, 5] = 0
    a = torch.randn((M, H), generator=torch.Generator().manual_seed(7)) / 4
    a[:, 5] = 25.0
    a = a.to(tdt)
    tw, ids = make_routing(M, E, K, seed=7)
    x = a.to(torch.float64).numpy()
    ref8 = ref_layer(x, w13, s13, w2, s2, ids, tw.astype(np.float64), "silu", tdt)
    # weight-only: T((q - 128) * T(s)) weights, 16-bit activations, fp32 kept up to the one rounding of the intermediate
    d13, d2 = rnd(w13 * rnd(s13, tdt)[..., None], tdt), rnd(w2 * rnd(s2, tdt)[..., None], tdt)
    ref16 = np.zeros_like(ref8)
    for e in range(E):
        m, k = np.nonzero(ids == e)
        g1 = x[m] @ d13[e].T
        h = rnd(g1[:, :I] / (1.0 + np.exp(-g1[:, :I])) * g1[:, I:], tdt)
        np.add.at(ref16, m, tw[m, k][:, None] * (h @ d2[e].T))
    return (M, E, K, H, I, tdt), (w13, s13, w2, s2), a, tw, ids, ref8, ref16


def far(out, ref):                                 # the share of elements outside the layer tolerance
    return (np.abs(out - ref) > 1e-2 * np.abs(ref).max() + 2e-2 * np.abs(ref)).mean()


def test_w8a16_case_separates_the_references():
    *_, ref8, ref16 = w8a16_case()
    assert far(ref16, ref8) > 0.5


@gpu
def test_mode_really_quantises_the_activations():
    (M, E, K, H, I, tdt), (w13, s13, w2, s2), a, tw, ids, ref8, _ = w8a16_case()
    args = (a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV))
    check(engine(w13, s13, w2, s2, tdt, K).decode(*args).cpu().numpy(), ref8, "W8A8")
    u8 = lambda w: (w.astype(np.int16) + 128).astype(np.uint8)                      # the same weights as uint8b128, act-dtype scales per 128 k
    sc = lambda s, k: torch.from_numpy(s).to(tdt)[..., None].repeat(1, 1, k // 128)
    from lvllm_amd.ops import RoutedExpertsEngine
    e16 = RoutedExpertsEngine(torch.from_numpy(u8(w13)), torch.from_numpy(u8(w2)), fmt="int8", w13_scale=sc(s13, H), w2_scale=sc(s2, I),
                              group_n=1, group_k=128, top_k=K, act_dtype=tdt, fp8_mode=_clib.FP8_W8A16)
    share = far(e16.decode(*args).cpu().numpy(), ref8)
    assert share > 0.5, f"the weight-only engine is within tolerance of the W8A8 reference on {1 - share:.0%} of the elements"


@gpu
@pytest.mark.parametrize("M,E,K,H,I", [(70, 8, 2, 512, 384), (300, 2, 1, 256, 128), (40, 2, 2, 1184, 1056)])
def test_plans_agree(M, E, K, H, I):
    """every tile height and every GEMM2 split-K give the same layer (GEMM2 of the first shape has 3 units, of the last 9: odd
    counts, slabs of unequal length); then one captured decode step, replayed"""
    eng = engine(*make_weights(np.random.default_rng(M), E, H, I, True), torch.bfloat16, K)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) / 4).to(torch.bfloat16).to(DEV)
    tw, ids = make_routing(M, E, K, seed=M, drop=0.05)
    twd, idd = torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    base = eng.decode(a, twd, idd).cpu().numpy()
    scale = np.abs(base).max()
    for kv in (dict(tiled=32), dict(tiled=64), dict(tiled=128), dict(tiled=256), dict(tiled=0, sk2=1), dict(sk2=2), dict(sk2=3)):
        eng.engine.set_tuning(**kv)
        out = eng.decode(a, twd, idd).cpu().numpy()
        print(kv, "max diff / scale:", np.abs(out - base).max() / scale)
        if kv.get("tiled"):                                                       # the forced height is the one that ran (TBW = height / 16)
            assert all(k.rsplit(", ", 2)[1] == str(kv["tiled"] // 16) for g_ in ("gemm1", "gemm2") for k in eng.engine.last_kernels()[g_]), eng.engine.last_kernels()
        np.testing.assert_allclose(out, base, atol=1e-5 * scale, rtol=0, err_msg=f"{kv} {eng.engine.describe()}")
    eng.engine.set_tuning(sk2=0)
    out = torch.empty((M, H), dtype=torch.float32, device=DEV)
    eng.decode(a, twd, idd, out=out)                                              # warm-up, then one captured decode step
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.decode(a, twd, idd, out=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("kw,zp,word", [(dict(fp8_mode=2), False, b"fp8_mode"), (dict(fp8_mode=1), True, b"zero points"),
                                        (dict(fp8_mode=1, groupK=64), False, b"groupK")])
def test_bad_arguments_are_refused_before_the_device_check(kw, zp, word):
    cfg = _clib.LkmConfig(**{**dict(abi_version=_clib.LKM_ABI_VERSION, has_gate_proj=1, expert_num=2, top_k=1, hidden_size=128, intermediate_size=64,
                                   groupN=1, groupK=128, weight_format=_clib.W_INT8, act_dtype=_clib.DT_BF16), **kw})
    buf, h = C.create_string_buffer(64), C.c_void_p()
    p = C.cast(buf, C.c_void_p)
    assert _clib.lib().lkm_create(C.byref(cfg), p, p, p, p, p if zp else None, p if zp else None, C.byref(h)) == _clib.E_INVALID
    assert word in _clib.lib().lkm_last_error()


def test_from_vllm_and_the_scheme_predicate():
    from lvllm_amd.modular import LkmExperts, LkmQuant
    s = torch.zeros((2, 8), dtype=torch.float32)
    qc = lambda **kw: types.SimpleNamespace(**{**dict(w1_scale=s, w2_scale=s, use_int8_w8a8=True, per_act_token_quant=True, block_shape=None,
                                                      a1_scale=None, a2_scale=None), **kw})
    q = LkmQuant.from_vllm(qc(), torch.bfloat16)
    assert (q.fmt, q.group_n, q.fp8_mode) == ("int8", 1, _clib.FP8_W8A8) and q.group_k >= 131072 and q.w1_scale is s
    for bad, word in ((dict(block_shape=[128, 128]), "block"), (dict(per_act_token_quant=False), "per-tensor"),
                      (dict(per_act_token_quant=False, a1_scale=s, a2_scale=s), "static")):
        with pytest.raises(ValueError, match=word):
            LkmQuant.from_vllm(qc(**bad), torch.bfloat16)
    wk, ak = "QuantKey(i8,scale(f32,static,per_channel),symmetric)", "QuantKey(i8,scale(f32,dynamic,per_token),symmetric)"
    assert LkmExperts._supports_quant_scheme(wk, ak)
    assert not LkmExperts._supports_quant_scheme("int8", "int8")
    assert not LkmExperts._supports_quant_scheme(wk, "QuantKey(i8,scale(f32,static,per_tensor),symmetric)")
