"""The chunk cases of tests/test_gpu_call_paths.py, run as a script in a fresh process: the scratch arena is per device and only
grows, so only a process that has built no larger engine sees the chunk sizes that these engines' own capacities give.  First
every configuration on engines sized for 48 tokens (`chunked`), then the activation-quantised ones after a larger 16-bit engine
has grown the shared slot arrays (`grown`).  One line `RESULT {json}` per case: case, ok, error, log (what the case printed)."""
import contextlib
import io
import json
import sys
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from tests import format_table as ft  # noqa: E402
from tests import test_gpu_call_paths as cp  # noqa: E402

M = 113


def chunked(name, family):
    """113 rows through an engine sized for 48: decode against the reference, lkm_prefill_host == decode bit for bit, the rows of
    the second chunk == a call on just those rows (the second chunk does not see the first chunk's scratch); and an engine
    configured with top_k = 2 called with K = 3 (the chunk is then cap_slots / 3 = 32 tokens)"""
    case = ft.make_case(name, family, seed=21)
    eng = case.engine(**cp.SMALL)
    a, (tw, ids) = ft.hidden(M, case.H, case.dt, 7), ft.routing(M, case.E, case.K, 7)
    ref = case.ref(a, ids, tw)
    ad, twd, idd = cp._dev(a, tw, ids)
    out = eng.decode(ad, twd, idd)
    d_all = eng.engine.describe()
    print(f"[{name}] 113 rows, last chunk: {d_all}")
    assert cp._last_m(d_all) == 17, d_all                                 # 48 + 48 + 17
    case.check(cp._f64(out), ref, "decode in chunks " + d_all)
    assert (cp._f64(out)[(ids < 0).all(axis=1)] == 0).all()
    host = eng.prefill_host(a, torch.from_numpy(tw), torch.from_numpy(ids))
    d_host = eng.engine.describe()
    print(f"[{name}] prefill_host: {d_host}")
    assert torch.equal(host.view(torch.int32), out.cpu().view(torch.int32)), (d_host, d_all)
    part = eng.decode(ad[48:96].contiguous(), twd[48:96].contiguous(), idd[48:96].contiguous())
    d_part = eng.engine.describe()
    cp._same(name, out[48:96], d_all, part, d_part, "rows [48, 96) of the chunked call against a call on those rows")
    two = eng.decode(ad[:96].contiguous(), twd[:96].contiguous(), idd[:96].contiguous())      # 48 + 48: the last chunk is those rows
    d_two = eng.engine.describe()
    assert cp._last_m(d_two) == 48, d_two
    cp._same(name, two[48:96], d_two, part, d_part, "the second of two whole chunks against a call on its rows")
    case3 = ft.make_case(name, family, seed=22)                           # K = 3 on an engine configured for top_k = 2
    eng3 = case3.engine(**cp.SMALL)
    tw3, ids3 = ft.routing(M, case.E, 3, 9)
    out3 = eng3.decode(ad, *cp._dev(tw3, ids3))
    d3 = eng3.engine.describe()
    print(f"[{name}] K=3: {d3}")
    assert cp._last_m(d3) == 17 and " K=3 " in d3, d3                     # 32 + 32 + 32 + 17
    case3.check(cp._f64(out3), case3.ref(a, ids3, tw3), "K=3 " + d3)


def grown(name):
    """an activation-quantised engine sized for 48 after the slot arrays were grown: its calls are still cut by its own scratch"""
    case = ft.make_case(name, "A", seed=23)
    eng = case.engine(**cp.SMALL)
    a, (tw, ids) = ft.hidden(M, case.H, case.dt, 8), ft.routing(M, case.E, case.K, 8)
    out = eng.decode(*cp._dev(a, tw, ids))
    desc = eng.engine.describe()
    print(f"[{name}] after the arena grew: {desc}")
    assert cp._last_m(desc) < M, desc
    case.check(cp._f64(out), case.ref(a, ids, tw), desc)


def run(key, fn, *args):
    log, err = io.StringIO(), ""
    try:
        with contextlib.redirect_stdout(log):
            fn(*args)
    except Exception:      # noqa: BLE001  (reported to the parent, which fails the case's test)
        err = traceback.format_exc()
    print("RESULT " + json.dumps(dict(case=key, ok=not err, error=err[-6000:], log=log.getvalue())), flush=True)
    return not err


def main():
    ok = True
    for name, family in ft.SHAPED:
        ok &= run(f"chunked {name} {family}", chunked, name, family)
    # a 16-bit engine sized for 512 tokens: 1024 slots, no quantised scratch
    big = ft.make_case("bf16", "A", seed=1).engine(max_num_seqs=8, max_batch_size=512, group_max_len=512)
    for name in ft.QUANTISED_ACTIVATIONS:
        ok &= run(f"grown {name}", grown, name)
    del big
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
