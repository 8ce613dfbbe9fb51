"""CPU: the format table (tests/format_table.py) builds every reference at family A without a GPU, and the inputs of the call-path
cases (tests/test_gpu_call_paths.py) meet the conditions those tests state."""
import numpy as np
import pytest
import torch

from tests import format_table as ft


def test_the_table_lists_every_engine_configuration():
    assert ft.NAMES == ["bf16", "f16", "int4", "int4fast", "int4zp", "int8", "int8zp", "int8a8", "fp8", "fp8a8", "mxfp4", "nvfp4",
                        "mxfp4a8", "mxfp4a4"]
    assert [n for n, fam in ft.SHAPED if fam == "B"] == ["bf16", "int8a8", "mxfp4a8", "mxfp4a4"]


@pytest.mark.parametrize("name", ft.NAMES)
def test_reference_runs_on_the_cpu(name):
    E, K, H = ft.FAMILY_A["E"], ft.FAMILY_A["K"], ft.FAMILY_A["H"]
    case = ft.make_case(name, "A", seed=3)
    M = 37
    a = ft.hidden(M, H, case.dt, 1)
    tw, ids = ft.routing(M, E, K, 1)
    assert not (ids == E - 1).any() and (ids < 0).any() and (ids >= 0).any()          # one expert empty, dropped slots
    ref = case.ref(a, ids, tw)
    assert ref.shape == (M, H) and np.isfinite(ref).all() and np.abs(ref).max() > 0
    dead = (ids < 0).all(axis=1)
    assert (ref[dead] == 0).all()
    # the reference tells two experts apart and depends on the inputs alone
    moved = case.ref(a, np.where(ids == 1, 2, ids).astype(np.int32), tw)
    assert (ids == 1).any() and not np.array_equal(moved, ref)
    np.testing.assert_array_equal(case.ref(a, ids, tw), ref)
    case.check(ref, ref, "reference against itself")
    # the local-window case on the same weights
    tw_w, gids, lids = ft.window_case(M, K, seed=5)
    assert ft.window_case_is_complete(gids, lids)
    ref_w = case.ref(a, lids, tw_w)
    none_local = (lids < 0).all(axis=1)
    assert none_local.any() and (ref_w[none_local] == 0).all() and np.abs(ref_w[~none_local]).max() > 0


@pytest.mark.parametrize("poison", ["max", "nan"])
def test_poisoned_views_hold_the_clean_rows(poison):
    M, E, K, H, dt = 37, 8, 2, 256, torch.bfloat16
    a = ft.hidden(M, H, dt, 2)
    tw, ids = ft.routing(M, E, K, 2)
    value = float("nan") if poison == "nan" else torch.finfo(dt).max
    (big_a, big_w, big_i), views = ft.strided_inputs(a, tw, ids, E, value)
    va, vw, vi = views(big_a, big_w, big_i)
    assert torch.equal(va, a) and np.array_equal(vw.numpy(), tw) and np.array_equal(vi.numpy(), ids)
    assert va.stride(0) == H + 24 and vw.stride(0) == K + 3 and vi.stride(0) == K + 3 and va.stride(0) % 8 == 0
    gap = torch.ones_like(big_a, dtype=torch.bool)
    gap[:, 8:8 + H] = False
    assert gap.sum() == M * 24
    assert torch.isnan(big_a[gap]).all() if poison == "nan" else (big_a[gap] == torch.finfo(dt).max).all()
    assert int((big_i == E + 7).sum()) == M * 3 and int((big_w == 1e30).sum()) == M * 3
