"""GPU: every engine configuration of tests/format_table.py through every door of the engine -- row-strided views
(lkm_forward_strided), a local expert window (id_offset), chunked calls and the host round trip (run_device / lkm_prefill_host),
the fused router (lkm_forward_routed), a captured step, expert images (lkm_export_expert / lkm_import_expert) -- against the
format's CPU reference at the format's own tolerance, and against the contiguous decode / prefill of the same rows.

Two calls of one engine on the same rows: where `engine.describe()` is the same after both, the results must agree bit for bit;
where the plans differ, fp32 results agree as tests/test_gpu_moe.py::_assert_same_math states (the exact-sum modes int8a8 /
mxfp4a8 / mxfp4a4: the 1e-5 of the scale of their test_plans_agree).  Every comparison prints both describe() strings.

The scratch arena is per device and only grows, so how a call is cut into chunks depends on the engines the process built before.
The chunk cases therefore run in a fresh child process (tests/call_path_chunks.py, started once per module): there a call of 113
rows on an engine sized for 48 is cut into 48 + 48 + 17, and the cases assert it.

Recorded on an MI355X, per table entry: strided fp32 / decode, strided activation dtype / prefill, the local window, the fused
router, the captured step, the host round trip and the second of two whole chunks against a call on its rows ran one plan
(equal describe()) and were bit for bit, for all 14 entries and both shape families.  Only rows [48, 96) of the 113-row call
against a call on those rows compared two describe() strings, the first showing the call's LAST chunk:
    family A (H=256):  "... | M=17 K=2 | tiled | ... tm=T waves=4 pd=P ..."  against  "... | M=48 K=2 | tiled | ... tm=T waves=4 pd=P ..."
        bf16, f16: T=64 P=4/4;  int4, int4fast, int4zp, mxfp4, nvfp4: T=32 P=2/4;  int8, int8zp, int8a8, mxfp4a8, mxfp4a4: T=32 P=2/2;
        fp8, fp8a8: "M=17 ... tm=32 pd=4/4" against "M=48 ... tm=64 pd=2/2"
    family B (H=160):  bf16 "M=17 K=2 | skinny | skinny g1 nt=1 tb=2 kw=1, g2 nt=1 tb=2 sk=1" against "M=48 K=2 | tiled | ... tm=64 pd=4/4";
        int8a8, mxfp4a8, mxfp4a4: "M=17 ... tm=32 pd=2/2" against "M=48 ... tm=64 pd=2/2"
and fell back to _assert_same_math (int8a8, mxfp4a8, mxfp4a4: 1e-5 of the scale)."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import format_table as ft
from tests.helpers import torch_to_bits
from tests.test_gpu_moe import _assert_same_math

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(max_num_seqs=8, max_batch_size=48, group_max_len=48)      # 48-token chunks where nothing larger was built before
PLAN_RTOL = {"int8a8": 0.0, "mxfp4a8": 1e-5, "mxfp4a4": 1e-5}          # the formats' test_plans_agree
FIRST, LOCAL, ROUTER_E = 4, 8, 16                                      # the local window of the id_offset cases
ROOT = Path(__file__).resolve().parents[1]


def _dev(*ts):
    return tuple((torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV) for t in ts)


def _f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _last_m(desc):
    return int(re.search(r"\| M=(\d+) K=\d+ \|", desc).group(1))


def _same(name, got, d_got, want, d_want, what):
    """the rule of the module docstring; got / want: device tensors of one dtype"""
    same_plan = d_got == d_want
    print(f"[{name}] {what}: {'bit for bit' if same_plan else 'same math'}\n    {d_got}\n    {d_want}")
    if same_plan:
        assert torch.equal(got.view(torch.int32 if got.dtype == torch.float32 else torch.int16),
                           want.view(torch.int32 if want.dtype == torch.float32 else torch.int16)), f"{name} {what}: {d_got}"
        return
    assert got.dtype == torch.float32, "two plans are compared on their fp32 results"
    g, w = _f64(got), _f64(want)
    scale = float(np.abs(w).max())
    if name in PLAN_RTOL:
        np.testing.assert_allclose(g, w, atol=1e-5 * scale, rtol=PLAN_RTOL[name], err_msg=f"{name} {what}")
    else:
        _assert_same_math(g, w, f"{name} {what}")


# --------------------------------------------------------------------------------------------------------------- chunks
@pytest.fixture(scope="module")
def chunk_results():
    """tests/call_path_chunks.py in a fresh child process, once: there no larger engine has grown the arena, so the chunk
    counts are what the engines' own sizes give"""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "call_path_chunks.py")], env=env, cwd=str(ROOT), capture_output=True, text=True,
                       timeout=600)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            rec = json.loads(line[len("RESULT "):])
            res[rec["case"]] = rec
    return r, res


def _chunk_case(chunk_results, key):
    r, res = chunk_results
    assert key in res, f"the child (exit code {r.returncode}) reported nothing for {key}:\n{r.stdout[-2000:]}{r.stderr[-3000:]}"
    print(res[key]["log"])
    assert res[key]["ok"], res[key]["error"]


@pytest.mark.parametrize("name,family", ft.SHAPED)
def test_chunked_calls_and_the_host_round_trip(chunk_results, name, family):
    """call_path_chunks.chunked: 113 rows through an engine sized for 48 (chunks of 48 + 48 + 17), against the reference, the host
    round trip and calls on the second chunk's rows; K = 3 on an engine configured for top_k = 2 (chunks of 32)"""
    _chunk_case(chunk_results, f"chunked {name} {family}")


@pytest.mark.parametrize("name", ft.QUANTISED_ACTIVATIONS)
def test_chunks_follow_the_formats_own_scratch_after_the_arena_grew(chunk_results, name):
    """call_path_chunks.grown: after a 16-bit engine sized for 512 tokens grew the shared slot arrays, an activation-quantised
    engine sized for 48 still cuts its calls by ITS scratch (quantised rows, scales, row sums)"""
    _chunk_case(chunk_results, f"grown {name}")


# --------------------------------------------------------------------------------------------------------- strided rows
@pytest.mark.parametrize("poison", ["max", "nan"])
@pytest.mark.parametrize("name,family", ft.SHAPED)
def test_strided_rows_between_poisoned_gaps(name, family, poison):
    """hidden rows inside [M, H + 24], ids and weights inside [M, K + 3]; the gaps hold the largest finite value / NaN, ids past the
    engine's experts and weights of 1e30: a quantiser, a row sum or a gather that reads past its columns changes the result"""
    M = 37
    case = ft.make_case(name, family, seed=11)
    eng = case.engine()
    a, (tw, ids) = ft.hidden(M, case.H, case.dt, 3), ft.routing(M, case.E, case.K, 3)
    ref = case.ref(a, ids, tw)
    value = float("nan") if poison == "nan" else torch.finfo(case.dt).max
    bigs, views = ft.strided_inputs(a, tw, ids, case.E, value)
    va, vw, vi = views(*_dev(*bigs))
    assert va.stride(0) == case.H + 24 and vw.stride(0) == case.K + 3 and vi.stride(0) == case.K + 3
    s32 = eng.forward_rows(va, vw, vi)
    d_s32 = eng.engine.describe()
    s16 = eng.forward_rows(va, vw, vi, out_dtype=case.dt)
    d_s16 = eng.engine.describe()
    ad, twd, idd = _dev(a, tw, ids)
    dec = eng.decode(ad, twd, idd)
    d_dec = eng.engine.describe()
    pre = eng.prefill(ad, twd, idd)
    d_pre = eng.engine.describe()
    case.check(_f64(s32), ref, "strided, fp32 out " + d_s32)
    case.check(_f64(s16), ref, "strided, activation-dtype out " + d_s16, rounded=True)
    assert s16.dtype == case.dt and (_f64(s32)[(ids < 0).all(axis=1)] == 0).all()
    _same(name, s32, d_s32, dec, d_dec, "strided fp32 against decode")
    if d_s16 == d_pre:
        _same(name, s16, d_s16, pre, d_pre, "strided activation dtype against prefill")
    else:       # two plans: their fp32 results were compared above, both activation-dtype results against the reference
        print(f"[{name}] strided activation dtype against prefill: plans differ\n    {d_s16}\n    {d_pre}")
        case.check(_f64(pre), ref, "prefill " + d_pre, rounded=True)


@pytest.mark.parametrize("name", ft.NAMES)
def test_local_expert_window(name):
    """global ids over 16 experts, the engine holds [4, 12): forward_rows(id_offset=4) == decode on the locally mapped ids"""
    M = 37
    case = ft.make_case(name, "A", seed=12)
    assert case.E == LOCAL
    eng = case.engine()
    a = ft.hidden(M, case.H, case.dt, 4)
    tw, gids, lids = ft.window_case(M, case.K, seed=5, router_experts=ROUTER_E, first=FIRST, local=LOCAL)
    assert ft.window_case_is_complete(gids, lids, FIRST, LOCAL)
    ad, twd, gd, ld = _dev(a, tw, gids, lids)
    out = eng.forward_rows(ad, twd, gd, id_offset=FIRST)
    d_out = eng.engine.describe()
    dec = eng.decode(ad, twd, ld)
    d_dec = eng.engine.describe()
    print(f"[{name}] window:\n    {d_out}\n    {d_dec}")
    assert torch.equal(out.view(torch.int32), dec.view(torch.int32)), (d_out, d_dec)
    case.check(_f64(out), case.ref(a, lids, tw), "local window " + d_out)
    none_local = (lids < 0).all(axis=1)
    assert none_local.any() and (_f64(out)[none_local] == 0).all()


# --------------------------------------------------------------------------------------------------------- fused router
def _logits(M, ldt, seed):
    return torch.randn((M, ROUTER_E), generator=torch.Generator().manual_seed(seed)).to(ldt)


def _oracle_router(logits, K):
    if logits.dtype == torch.float32:
        return orc.topk_softmax(logits.numpy(), K, renormalize=True)
    return orc.topk_softmax(torch_to_bits(logits), K, dt=orc.BF16, renormalize=True)


def _to_local(gids):
    return np.where((gids >= FIRST) & (gids < FIRST + LOCAL), gids - FIRST, -1).astype(np.int32)


@pytest.mark.parametrize("name", ft.NAMES)
def test_fused_router_equals_router_then_forward(name):
    """lkm_forward_routed == lkm_topk_softmax then lkm_forward_strided, bit for bit in out, weights and ids (include/lkm.h): one
    token and three (routing inside GEMM1 where the plan is direct), forty (router inside the sort launch); with the fused launch
    and with the two-call fallback ("fuse" = -1); the router's outputs equal the oracle router, the layer matches the reference"""
    from lvllm_amd import ops
    case = ft.make_case(name, "A", seed=13)
    eng = case.engine()
    K = case.K
    for M in (1, 3, 40):
        for ldt in (torch.float32, torch.bfloat16):
            a, logits = ft.hidden(M, case.H, case.dt, 10 + M), _logits(M, ldt, 20 + M)
            wr, ir = _oracle_router(logits, K)
            ref = case.ref(a, _to_local(ir), wr)
            ad, lg = _dev(a, logits)
            w0, i0 = ops.topk_softmax(lg, K, True)
            np.testing.assert_array_equal(i0.cpu().numpy(), ir)
            np.testing.assert_array_equal(w0.cpu().numpy().view(np.int32), wr.view(np.int32))
            for fuse in (0, -1):
                eng.engine.set_tuning(fuse=fuse)
                out, w, ids = eng.forward_logits(ad, lg, K, True, id_offset=FIRST)
                d_out = eng.engine.describe()
                base = eng.forward_rows(ad, w0, i0, id_offset=FIRST)
                what = f"M={M} logits={ldt} fuse={fuse}"
                print(f"[{name}] {what}:\n    {d_out}\n    {eng.engine.describe()}")
                assert torch.equal(ids, i0) and torch.equal(w.view(torch.int32), w0.view(torch.int32)), what
                assert torch.equal(out.view(torch.int32), base.view(torch.int32)), (what, d_out, eng.engine.describe())
                case.check(_f64(out), ref, what + " " + d_out)
    eng.engine.set_tuning(fuse=0)


@pytest.mark.parametrize("name", ft.NAMES)
def test_captured_routed_step_follows_new_logits(name):
    """one lkm_forward_routed step captured on a side stream after a warm-up; replayed, then replayed after the logits were
    overwritten in place: every replay equals the eager call on the same logits bit for bit"""
    M = 24
    case = ft.make_case(name, "A", seed=14)
    eng = case.engine()
    K = case.K
    a = ft.hidden(M, case.H, case.dt, 6)
    first, second = _logits(M, torch.float32, 31), _logits(M, torch.float32, 32)
    ad, lg, lg2 = _dev(a, first, second)
    out = torch.empty((M, case.H), dtype=torch.float32, device=DEV)
    eager, w_e, i_e = eng.forward_logits(ad, lg, K, True, id_offset=FIRST)
    d_eager = eng.engine.describe()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.forward_logits(ad, lg, K, True, id_offset=FIRST, out=out)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        _, w_g, i_g = eng.forward_logits(ad, lg, K, True, id_offset=FIRST, out=out)
    print(f"[{name}] captured step:\n    {d_eager}\n    {eng.engine.describe()}")
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and torch.equal(i_g, i_e) and torch.equal(w_g, w_e)
    wr, ir = _oracle_router(first, K)
    case.check(_f64(out), case.ref(a, _to_local(ir), wr), "replay " + d_eager)
    lg.copy_(lg2)                                                         # new logits in the captured buffer
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        got, w2, i2 = out.clone(), w_g.clone(), i_g.clone()
        eager2, w_e2, i_e2 = eng.forward_logits(ad, lg, K, True, id_offset=FIRST)
        assert not torch.equal(i_e2, i_e)
        assert torch.equal(got.view(torch.int32), eager2.view(torch.int32)) and torch.equal(i2, i_e2) and torch.equal(w2, w_e2)


# -------------------------------------------------------------------------------------------------------- expert images
def _all_on(eng, x, expert):
    M = x.size(0)
    return eng.decode(x, torch.ones((M, 1), dtype=torch.float32, device=DEV), torch.full((M, 1), expert, dtype=torch.int32, device=DEV)).clone()


IMAGE_CASES = [(n, f, True) for n, f in ft.SHAPED] + [(n, f, False) for n in ft.NAMES if ft.FORMATS[n].relu2_images for f in "AB"]


def _moved(name, family, gated):
    """slot 1 -> slot 2 within one engine, then expert 3 of it -> slot 0 of a second engine of the same configuration"""
    from lvllm_amd.eplb import EngineExpertStore
    M = 19
    case, other = ft.make_case(name, family, gated, seed=31), ft.make_case(name, family, gated, seed=32)
    eng, oth = case.engine(), other.engine()
    st, st2 = EngineExpertStore(eng), EngineExpertStore(oth)
    a = ft.hidden(M, case.H, case.dt, 5)
    x, = _dev(a)
    before = [_all_on(eng, x, e) for e in range(case.E)]
    img = torch.empty(st.expert_nbytes, dtype=torch.uint8, device=DEV)
    st.export_expert(1, img)
    st.import_expert(2, img)
    after = [_all_on(eng, x, e) for e in range(case.E)]
    st.export_expert(3, img)
    st2.import_expert(0, img)
    img2 = torch.empty_like(img)                                          # export after import returns the imported bytes
    st2.export_expert(0, img2)
    return dict(case=case, other=other, eng=eng, oth=oth, st=st, st2=st2, a=a, x=x, before=before, after=after, img=img, img2=img2)


@pytest.mark.parametrize("name,family,gated", IMAGE_CASES)
def test_expert_image_moves_an_expert(name, family, gated):
    """the body of tests/test_zz3_gpu_eplb.py::test_expert_image_moves_an_expert_bit_for_bit for every configuration (non-gated
    layers halve every w13 slab)"""
    m = _moved(name, family, gated)
    E, st, st2, before, after = m["case"].E, m["st"], m["st2"], m["before"], m["after"]
    assert st.num_local == E and st.expert_nbytes == st2.expert_nbytes and st.expert_nbytes % 16 == 0
    assert st.expert_nbytes * E >= m["eng"].engine.weight_bytes() - 64   # the images cover the weight buffers
    assert not torch.equal(before[1], before[2])
    assert torch.equal(after[2], before[1])                               # within one engine; the other slots untouched
    for e in range(E):
        assert e == 2 or torch.equal(after[e], before[e]), e
    assert torch.equal(_all_on(m["oth"], m["x"], 0), before[3])           # across engines
    assert torch.equal(m["img"], m["img2"])


# fp8a8 at family A, the oracle comparison of the moved expert only (the bit-for-bit assertions above run unmarked): 1 of the 4864
# outputs, [14, 43], is 0.00440 from the reference where the format's tolerance allows 0.00387 + 0.02 |ref| (max|ref| = 0.387).
# The cause, from a float64 restatement of row 14 that reproduces the oracle's row exactly: the exact GEMM1 gate sum of element
# 111 is 0.548829439, 1.3e-6 (3.4e-4 of a bf16 ulp, the size of an fp32 summation-order difference over 256 products) above
# the bf16 tie 0.548828125.  The oracle rounds it up to 0.55078, the kernel's sum falls below the tie; after the two roundings of
# the activation the intermediate is 0.2119 instead of 0.2148, which with the group's scale (amax 0.4766 / 448) is 199.2 instead
# of 202.0, on the other side of the fp8 boundary 200: code 192 instead of 208.  The row's difference from the oracle is -1.000
# times that one fp8 step (0.01702) times column 111 of w2, with a residual at the level of the other rows (the bf16 rounding of
# the oracle's output); rows 5, 6 and 16 show the same with smaller steps, inside the tolerance.  Neither side is wrong, and one
# such step on a large element of the intermediate is about 1 % of the output scale, which is the tolerance's atol.
_FP8A8_REF = pytest.mark.xfail(strict=True, reason="fp8a8: output [14, 43] of 4864 is 0.00440 from the oracle, tolerance 0.00426: the GEMM1 sum of one "
                               "element lies 3.4e-4 bf16 ulp from a tie, the kernel's fp32 sum rounds the other way and the intermediate "
                               "moves by one fp8 step (code 192 for 208); see the comment above")


@pytest.mark.parametrize("name,family,gated", [pytest.param(n, f, g, marks=[_FP8A8_REF] if (n, f, g) == ("fp8a8", "A", True) else []) for n, f, g in IMAGE_CASES])
def test_moved_expert_matches_the_reference(name, family, gated):
    """an expert moved by its image computes what the reference computes with that expert's weights, in its new slot of the same
    engine and in another engine; the other engine's remaining slots keep their own weights"""
    m = _moved(name, family, gated)
    case, other, a, x, M = m["case"], m["other"], m["a"], m["x"], m["a"].shape[0]
    on = lambda e: (np.full((M, 1), e, np.int32), np.ones((M, 1), np.float32))
    case.check(_f64(_all_on(m["oth"], x, 0)), case.ref(a, *on(3)), "expert 3 in slot 0 of the other engine")
    other.check(_f64(_all_on(m["oth"], x, 1)), other.ref(a, *on(1)), "the other engine's slot 1 is untouched")
    case.check(_f64(m["after"][2]), case.ref(a, *on(1)), "expert 1 in slot 2 " + m["eng"].engine.describe())
