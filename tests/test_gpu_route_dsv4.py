"""DeepSeek-V4 routing (lkm_topk_route / lkm_forward_routed_ex): sqrtsoftplus scores, hash-table ids, padding rows, against a float64
restatement of fused_topk_bias_router.py:75-118.  Ids exact and in order; weights at atol = rtol = 2e-5, the reference's own bound
for its DeepSeek-V4 top-k.  _ref asserts its margin: a gap among the top K + 1 choices is 0 (the lowest index wins) or above 1e-5,
five times the fp32 error of a choice value (a few ulp of <= 5, about 2e-6)."""
import types

import numpy as np
import pytest
import torch

from lvllm_amd import ops
from lvllm_amd.layer import RoutedExpertsLayer, RoutingConfig
from tests import format_table as ft

gpu = pytest.mark.gpu
DEV, M, TOL, SQ = "cuda:0", 37, 2e-5, "sqrtsoftplus"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _inputs(m, E, K, dt, seed=0, vocab=64):           # -> logits [m, E], bias fp32 [E], hash table [vocab, K], token ids [m]
    g = torch.Generator().manual_seed(seed)
    logits, bias = torch.randn((m, E), generator=g).to(dt), torch.randn((E,), generator=g)
    return logits, bias, torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(vocab)]), torch.randint(0, vocab, (m,), generator=g)


def _ref(logits, K, bias=None, renorm=True, scale=1.0, table=None, tokens=None):
    s = np.sqrt(np.logaddexp(0.0, logits.to(torch.float64).numpy()))
    if table is None:
        c = s if bias is None else s + bias.to(torch.float64).numpy()
        order = np.argsort(-c, axis=1, kind="stable")
        top = np.take_along_axis(c, order[:, :K + 1], 1)
        assert ((top[:, :-1] == top[:, 1:]) | (top[:, :-1] - top[:, 1:] > 1e-5)).all(), "the inputs leave no margin for fp32 scores"
        ids = order[:, :K]
    else:           # the table's rows as they stand; a token outside the table voids the row, an entry outside the experts its slot
        ok = ((tokens >= 0) & (tokens < table.size(0))).numpy()
        ids = table[tokens.clamp(0, table.size(0) - 1)].numpy().copy()
        ids[(ids < 0) | (ids >= s.shape[1]) | ~ok[:, None]] = -1
    w = np.where(ids >= 0, np.take_along_axis(s, np.maximum(ids, 0), 1), 0.0)
    den = w.sum(1, keepdims=True) if renorm else 1.0
    return w / np.where(den > 0, den, 1.0) * scale, ids.astype(np.int32)


def _check(got, want, pad=None):
    w, ids = (t.cpu().numpy() for t in got)
    if pad is not None:                                 # padding rows: ids -1 and weights +0.0; `want` holds the other rows
        assert (ids[pad] == -1).all() and (w[pad].view(np.int32) == 0).all()
        w, ids = w[~pad], ids[~pad]
    np.testing.assert_array_equal(ids, want[1])
    np.testing.assert_allclose(w.astype(np.float64), want[0], atol=TOL, rtol=TOL)


@gpu
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("E", [16, 64, 96, 256, 384, 512])
def test_selection(E, dt, with_bias):
    """every (slots, lanes per row) shape of the router: the bias chooses, the weight is the unbiased score"""
    K = {16: 6, 512: 16}.get(E, 8)
    logits, bias, _, _ = _inputs(M, E, K, DT[dt])
    for renorm, scale in ((True, 1.5), (False, 1.0)):
        got = ops.fused_topk_bias(logits.to(DEV), logits.to(DEV), bias.to(DEV) if with_bias else None, K, renorm, SQ, scale)
        _check(got, _ref(logits, K, bias if with_bias else None, renorm, scale))


@gpu
def test_selection_behind_the_gate_projection():
    g = torch.Generator().manual_seed(0)
    x, gw, bias = (torch.randn((M, 64), generator=g) / 4).bfloat16(), (torch.randn((96, 64), generator=g) / 2).bfloat16(), torch.randn((96,), generator=g)
    w, ids, logits = ops.router_topk(x.to(DEV), gw.to(DEV), 8, True, scoring_func=SQ, e_score_correction_bias=bias.to(DEV), return_logits=True)
    _check((w, ids), _ref(logits.cpu(), 8, bias))


@gpu
@pytest.mark.parametrize("tdt", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("E,K", [(64, 5), (256, 6), (384, 8), (512, 16)])
def test_hash(E, K, dt, tdt):
    """ids are the table's rows; one token past the vocabulary (row 3) and one table entry past E (in row 5)"""
    logits, _, table, tokens = _inputs(M, E, K, DT[dt])
    tokens[3], table[tokens[5], 1] = table.size(0) + 3, E + 7
    for renorm, scale in ((True, 1.5), (False, 1.0)):
        want = _ref(logits, K, None, renorm, scale, table, tokens)
        _check(ops.topk_softmax(logits.to(DEV), K, renorm, None, SQ, scale, input_tokens=tokens.to(tdt).to(DEV),
                                hash_indices_table=table.to(tdt).to(DEV)), want)


@gpu
@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("E", [16, 64])
def test_padding(E, hashed):
    """masked rows hold NaN logits and come out as (-1, +0.0); at E = 16 and in hashed rows they share a wavefront with live rows"""
    logits, _, table, tokens = _inputs(8, E, 6, torch.float32)
    pad = torch.arange(8) % 2 == 1
    logits[pad] = float("nan")
    got = ops.topk_softmax(logits.to(DEV), 6, True, None, SQ, is_padding=pad.to(DEV),
                           **(dict(input_tokens=tokens.to(DEV), hash_indices_table=table.to(DEV)) if hashed else {}))
    _check(got, _ref(logits[~pad], 6, table=table if hashed else None, tokens=tokens[~pad]), pad.numpy())


@gpu
@pytest.mark.parametrize("variant", ["bias", "hash", "hash+pad"])
@pytest.mark.parametrize("m", [1, 3, 37])
def test_fused_step_equals_router_then_engine(m, variant):
    """lkm_forward_routed_ex == lkm_topk_route then lkm_forward_strided, bit for bit (8 bf16 experts behind ids 4..11 of a 16-expert
    router): routed inside GEMM1 (M = 1, 3) and inside the sort launch (37); padding rows (0, 2, ...) come out as zeros; M = 3 also captured"""
    case = ft.make_case("bf16", "A", seed=13)
    eng, x = case.engine(), ft.hidden(m, case.H, case.dt, 10 + m).to(DEV)
    logits, bias, table, tokens = _inputs(m, 16, case.K, torch.float32, seed=m)
    pad = (torch.arange(m) % 2 == 0) & (variant == "hash+pad")
    logits[pad] = float("nan")
    logits, pad = logits.to(DEV), pad.to(DEV)
    kw = dict(e_score_correction_bias=bias.to(DEV)) if variant == "bias" else dict(input_tokens=tokens.to(DEV), hash_indices_table=table.to(DEV))
    kw.update(dict(is_padding=pad) if variant == "hash+pad" else {})
    w0, i0 = ops.topk_softmax(logits, case.K, True, scoring_func=SQ, routed_scaling_factor=1.5, **kw)
    base = eng.forward_rows(x, w0, i0, id_offset=4)
    call = lambda **o: eng.forward_logits(x, logits, case.K, True, scoring_func=SQ, routed_scaling_factor=1.5, id_offset=4, **kw, **o)  # noqa: E731
    out, w, ids = call()
    assert torch.equal(ids, i0) and torch.equal(w.view(torch.int32), w0.view(torch.int32)) and torch.equal(out.view(torch.int32), base.view(torch.int32)), eng.engine.describe()
    assert (ids[~pad] >= 0).all() and (ids[pad] == -1).all() and (out[pad].view(torch.int32) == 0).all()
    if m == 3 and variant != "bias":
        s, gr = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(gr, stream=s):
            _, w_g, i_g = call(out=out)
        for _ in range(3):
            out.fill_(7.0), w_g.fill_(7.0), i_g.fill_(7)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), base.view(torch.int32)) and torch.equal(i_g, i0) and torch.equal(w_g, w0)


def test_refusals_and_layer_keywords_on_the_cpu():
    """an unknown scoring name and grouped sqrtsoftplus raise; a layer passes the new keywords to its ops only when they are given"""
    x, logits, seen = torch.zeros((2, 8), dtype=torch.bfloat16), torch.zeros((2, 4)), []
    for match, bad in (("Unsupported scoring", lambda: ops.topk_softmax(logits, 2, True, None, "softplus")),
                       ("group-limited", lambda: ops.grouped_topk(x, logits, 2, True, 2, 1, SQ)),
                       ("group-limited", lambda: RoutingConfig(2, 4, scoring_func=SQ, use_grouped_topk=True, num_expert_group=2, topk_group=1))):
        with pytest.raises(ValueError, match=match):
            bad()

    def topk_softmax(logits, K, renorm, bias=None, scoring="softmax", scale=1.0, **kw):
        seen.append(sorted(kw))
        return torch.ones((2, K)), torch.zeros((2, K), dtype=torch.int32)
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(max_num_seqs=4), decode=lambda x, tw, ids, out=None: out.zero_())
    cfg = RoutingConfig(2, 4, scoring_func=SQ, hash_indices_table=torch.zeros((5, 2), dtype=torch.int64))
    for routing, kw in ((RoutingConfig(2, 4), {}), (cfg, dict(input_ids=torch.zeros(2, dtype=torch.int64), is_padding=torch.zeros(2, dtype=torch.bool)))):
        RoutedExpertsLayer(eng, routing, ops=types.SimpleNamespace(topk_softmax=topk_softmax)).forward(x, logits, **kw)
    assert seen == [[], ["hash_indices_table", "input_tokens", "is_padding"]] and cfg.hash_indices_table.dtype == torch.int32
