"""MXFP4 weights x MXFP8 activations (LKM_W_MXFP4 with fp8_mode = LKM_FP8_W8A8: gemm_mxa8_kernel on the scaled MFMA) against a
float64 restatement of the mode's numerics: MXFP8 quantiser bytes, the operand layout on one tile, whole layers, plan parity."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from lvllm_amd import _clib
from tests.helpers import make_routing

gpu = pytest.mark.gpu
DEV = "cuda:0"
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
ACTS = {"silu": dict(activation_type=0), "swigluoai": dict(activation_type=1), "relu2": dict(activation_type=2, has_gate_proj=False)}


def rnd(x, tdt):                                   # float64 -> the activation dtype (RNE) -> float64
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(tdt).to(torch.float64).numpy()


def mxq(x):
    """x float64 [R, K] (16-bit values) -> (e4m3fn bytes [R, K], E8M0 bytes [R, K / 32], dequantised float64 [R, K])"""
    R, K = x.shape
    b = x.reshape(R, K // 32, 32)
    amax = np.abs(b).max(-1)
    m, ex = np.frexp(amax)                         # amax = (2 m) 2^(ex - 1), 2 m in [1, 2)
    byte = np.clip(np.where(2 * m <= 1.75, ex - 9, ex - 8) + 127, 0, 254)
    byte[amax == 0] = 0
    q = torch.from_numpy(b * 2.0 ** (127 - byte)[..., None]).to(torch.float32).to(torch.float8_e4m3fn)
    deq = q.to(torch.float64).numpy() * 2.0 ** (byte - 127)[..., None]
    return q.view(torch.uint8).numpy().reshape(R, K), byte.astype(np.uint8), deq.reshape(R, K)


def deq_w(q, s):                                   # E2M1 bytes [E, N, K / 2] (even k low) + E8M0 [E, N, K / 32] -> float64 [E, N, K]
    w = np.stack([E2M1[q & 15], E2M1[q >> 4]], -1).reshape(*q.shape[:2], -1)
    return w * np.repeat(2.0 ** (s.astype(np.int64) - 127), 32, -1)


def ref_layer(a, w13, w2, ids, tw, act, tdt):
    """the specification: MXFP8 tokens, fp32-exact GEMM1 rounded to tdt, activation on the rounded value, rounded, MXFP8 along I,
    GEMM2, router weights"""
    x = mxq(a)[2]
    out = np.zeros((a.shape[0], w2.shape[1]))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    for e in range(w13.shape[0]):
        m, k = np.nonzero(ids == e)
        if not len(m):
            continue
        g1 = rnd(x[m] @ w13[e].T, tdt)
        if act == "silu":
            I = g1.shape[1] // 2
            h = rnd(g1[:, :I] * sig(g1[:, :I]), tdt) * g1[:, I:]
        elif act == "swigluoai":
            g, u = np.minimum(g1[:, 0::2], 7.0), np.clip(g1[:, 1::2], -7.0, 7.0)
            h = (u + 1.0) * g * sig(g * 1.702)
        else:
            h = np.maximum(g1, 0.0) ** 2
        h = rnd(h, tdt)
        np.add.at(out, m, tw[m, k][:, None] * (mxq(h)[2] @ w2[e].T))
    return out


def make_weights(rng, E, H, I, gated):             # random E2M1 codes, E8M0 scales 2^-9 .. 2^-5 -> (q13, q2, s13, s2)
    n13 = (2 if gated else 1) * I
    q13, q2 = rng.integers(0, 256, (E, n13, H // 2), dtype=np.uint8), rng.integers(0, 256, (E, H, I // 2), dtype=np.uint8)
    s13, s2 = rng.integers(118, 123, (E, n13, H // 32), dtype=np.uint8), rng.integers(118, 123, (E, H, I // 32), dtype=np.uint8)
    return q13, q2, s13, s2


def engine(q13, q2, s13, s2, tdt, K, act="silu", fp8_mode=_clib.FP8_W8A8, **kw):
    from lvllm_amd.ops import RoutedExpertsEngine
    return RoutedExpertsEngine(torch.from_numpy(q13), torch.from_numpy(q2), fmt="mxfp4", w13_scale=torch.from_numpy(s13),
                               w2_scale=torch.from_numpy(s2), group_n=1, group_k=32, top_k=K, act_dtype=tdt, fp8_mode=fp8_mode, **ACTS[act], **kw)


def make_layer(rng, E, H, I, gated, tdt, fp8_mode=_clib.FP8_W8A8, K=2, act="silu"):
    q13, q2, s13, s2 = make_weights(rng, E, H, I, gated)
    return engine(q13, q2, s13, s2, tdt, K, act, fp8_mode), deq_w(q13, s13), deq_w(q2, s2)


def check(out, ref, what=""):                     # the W8A8 tolerance of tests/test_gpu_moe.py, every element
    err = np.abs(out - ref)
    print(f"{what} max|ref|={np.abs(ref).max():.4g} max err={err.max():.4g} differing={int((err > 0).sum())}/{err.size}")
    np.testing.assert_allclose(out, ref, atol=1e-2 * np.abs(ref).max(), rtol=2e-2, err_msg=what)


@gpu
@pytest.mark.parametrize("rows,cols,ld", [(1, 32, 32), (5, 160, 168), (33, 4096, 4096)])
@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16])
def test_quantiser_bytes_exact(tdt, rows, cols, ld):
    from lvllm_amd import ops
    x = torch.randn((rows, ld), generator=torch.Generator().manual_seed(cols)).to(tdt)
    step_above = float(torch.nextafter(torch.tensor(1792.0, dtype=tdt), torch.tensor(float("inf"), dtype=tdt)))
    # edge blocks by their maximum: all zero, exactly 448 * 2^k, one step above that, fp16 subnormals, the largest finite value
    # (each in its own block of the two larger shapes; the single block of (1, 32) can hold only the last of them)
    for i, peak in enumerate([0.0, 448 * 2.0 ** -3, step_above, 3 * 2.0 ** -24, torch.finfo(tdt).max]):
        r, c = (i * 7) % rows, ((i * 3) % (cols // 32)) * 32
        x[r, c:c + 32] = (torch.rand(32, generator=torch.Generator().manual_seed(i)) * 0.4 * peak).to(tdt)
        x[r, c + 5 + i] = peak
    x = x[:, :cols]
    q, s = ops.quant_mxfp8_rows(x.to(DEV))
    rq, rs, _ = mxq(x.to(torch.float64).numpy())
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    np.testing.assert_array_equal(q.cpu().numpy(), rq)


@gpu
@pytest.mark.parametrize("M", [1, 16])
def test_one_tile_pins_operand_layout(M):
    from lvllm_amd.ops import RoutedExpertsEngine
    H, I, tdt = 128, 32, torch.bfloat16
    rng = np.random.default_rng(M)
    q13 = rng.integers(0, 256, (1, 2 * I, H // 2), dtype=np.uint8)                 # a distinct nibble pattern per row ...
    s13 = (116 + (np.arange(2 * I)[:, None] * 5 + np.arange(4)[None, :] * 3) % 12).astype(np.uint8)[None]   # ... and scale per (row, block)
    q2 = np.zeros((1, H, I // 2), np.uint8)                                        # w2: +1.0 at column h % I of output row h
    q2[0, np.arange(H), (np.arange(H) % I) // 2] = np.where(np.arange(H) % 2, 0x20, 0x02)
    s2 = np.full((1, H, 1), 127, np.uint8)
    eng = RoutedExpertsEngine(torch.from_numpy(q13), torch.from_numpy(q2), fmt="mxfp4", w13_scale=torch.from_numpy(s13), w2_scale=torch.from_numpy(s2),
                              group_n=1, group_k=32, top_k=1, act_dtype=tdt, fp8_mode=_clib.FP8_W8A8)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) * torch.linspace(0.05, 2.0, H)).to(tdt)
    ids, tw = np.zeros((M, 1), np.int32), np.ones((M, 1), np.float32)
    out = eng.decode(a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)).cpu().numpy()
    check(out, ref_layer(a.to(torch.float64).numpy(), deq_w(q13, s13), deq_w(q2, s2), ids, tw, "silu", tdt), eng.engine.describe())


# the last shape: K loops longer than one trip of four units and no multiple of it (GEMM1 10 units, GEMM2 9): the steady loop, its
# scale-dword hand-over between groups, and a drain of 2 / 1 units
SHAPES = [(1, 4, 2, 160, 96), (17, 4, 2, 160, 96), (130, 2, 1, 256, 128), (70, 8, 2, 512, 384), (33, 4, 2, 1184, 1056)]


@gpu
@pytest.mark.parametrize("M,E,K,H,I,act,tdt", [(*s, act, torch.bfloat16) for s in SHAPES for act in ACTS] +
                         [(*SHAPES[1], act, torch.float16) for act in ACTS])
def test_whole_layer(M, E, K, H, I, act, tdt):
    eng, w13, w2 = make_layer(np.random.default_rng(M + H), E, H, I, act != "relu2", tdt, K=K, act=act)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) / 4).to(tdt)
    tw, ids = make_routing(M, E, K, seed=M, drop=0.1)
    ids[ids == E - 1] = -1                                                        # one expert stays empty
    if M == 130:
        ids[:] = 0                                                                # every token on expert 0: 130 rows cross the 128-row tile
    ref = ref_layer(a.to(torch.float64).numpy(), w13, w2, ids, tw.astype(np.float64), act, tdt)
    ad, twd, idd = a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    check(eng.decode(ad, twd, idd).cpu().numpy(), ref, "decode " + eng.engine.describe())
    assert all("gemm_mxa8_kernel" in k for g in ("gemm1", "gemm2") for k in eng.engine.last_kernels()[g]), eng.engine.last_kernels()
    check(eng.prefill(ad, twd, idd).float().cpu().numpy(), rnd(ref, tdt), "gpu_prefill")


@gpu
def test_mode_is_really_w4a8():
    M, E, K, H, I, tdt = 17, 4, 2, 256, 128, torch.bfloat16
    a = torch.randn((M, H), generator=torch.Generator().manual_seed(7)) / 48
    # one element ~200 x the rest in every 32-block, at 1.0625 * 2^2: a tie of the e4m3 grid (-> 4.0), exact in bf16.  These elements
    # carry GEMM1, so MXFP8 moves gate and up by -5.9 % each and the layer by ~11 %; the small ones land on a grid of 1/8 .. 1/4
    a[:, 5::32] = 4.25 * torch.sign(a[:, 5::32])
    a = a.to(tdt)
    tw, ids = make_routing(M, E, K, seed=7)
    outs = {}
    for mode in (_clib.FP8_W8A8, _clib.FP8_W8A16):
        eng, w13, w2 = make_layer(np.random.default_rng(9), E, H, I, True, tdt, fp8_mode=mode, K=K)
        outs[mode] = eng.decode(a.to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)).cpu().numpy()
    ref = ref_layer(a.to(torch.float64).numpy(), w13, w2, ids, tw.astype(np.float64), "silu", tdt)
    check(outs[_clib.FP8_W8A8], ref, "W4A8")
    far = np.abs(outs[_clib.FP8_W8A16] - ref) > 1e-2 * np.abs(ref).max() + 2e-2 * np.abs(ref)
    assert far.mean() > 0.5, f"the weight-only engine is within tolerance of the W4A8 reference on {1 - far.mean():.0%} of the elements"


@gpu
@pytest.mark.parametrize("M,E,K,H,I", [(70, 8, 2, 512, 384), (300, 2, 1, 256, 128), (40, 2, 2, 1184, 1056)])
def test_plans_agree(M, E, K, H, I):
    """every tile height and every GEMM2 split-K give the same layer (the last shape has 9 GEMM2 units = 3 groups of four: slabs
    that start past the first group; a split wider than the groups is cut to them).  The intermediate's quantisation exists in
    one form only, the separate pass, so there is no fused form to compare yet."""
    eng, _, _ = make_layer(np.random.default_rng(M), E, H, I, True, torch.bfloat16, K=K)
    a = (torch.randn((M, H), generator=torch.Generator().manual_seed(M)) / 4).to(torch.bfloat16).to(DEV)
    tw, ids = make_routing(M, E, K, seed=M, drop=0.05)
    twd, idd = torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    base = eng.decode(a, twd, idd).cpu().numpy()
    scale = np.abs(base).max()
    for kv in (dict(tiled=32), dict(tiled=64), dict(tiled=128), dict(tiled=256), dict(tiled=0, sk2=1), dict(sk2=2), dict(sk2=3)):
        eng.engine.set_tuning(**kv)
        out = eng.decode(a, twd, idd).cpu().numpy()
        print(kv, "max diff / scale:", np.abs(out - base).max() / scale)
        np.testing.assert_allclose(out, base, atol=1e-5 * scale, rtol=1e-5, err_msg=f"{kv} {eng.engine.describe()}")
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


def test_bad_fp8_mode_is_refused_before_the_device_check():
    cfg = _clib.LkmConfig(abi_version=_clib.LKM_ABI_VERSION, has_gate_proj=1, expert_num=2, top_k=1, hidden_size=128, intermediate_size=64,
                          groupN=1, groupK=32, weight_format=_clib.W_MXFP4, act_dtype=_clib.DT_BF16, fp8_mode=2)
    buf, h = C.create_string_buffer(64), C.c_void_p()
    p = C.cast(buf, C.c_void_p)
    assert _clib.lib().lkm_create(C.byref(cfg), p, p, p, p, None, None, C.byref(h)) == _clib.E_INVALID
    assert b"fp8_mode" in _clib.lib().lkm_last_error()


def test_from_vllm_maps_the_mode():
    from lvllm_amd.modular import LkmExperts, LkmQuant
    s = torch.zeros((2, 4, 4), dtype=torch.uint8)
    a8 = LkmQuant.from_vllm(types.SimpleNamespace(w1_scale=s, w2_scale=s, weight_quant_dtype="mxfp4", quant_dtype="mxfp8"), torch.bfloat16)
    a16 = LkmQuant.from_vllm(types.SimpleNamespace(w1_scale=s, w2_scale=s, use_mxfp4_w4a16=True), torch.bfloat16)
    assert (a8.fmt, a8.group_n, a8.group_k, a8.fp8_mode) == ("mxfp4", 1, 32, _clib.FP8_W8A8)
    assert (a16.fmt, a16.fp8_mode) == ("mxfp4", _clib.FP8_W8A16)
    assert LkmExperts._supports_quant_scheme("mxfp4", "mxfp8") and LkmExperts._supports_quant_scheme("mxfp4", None)
    assert not LkmExperts._supports_quant_scheme("nvfp4", "mxfp8")
