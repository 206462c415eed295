"""Every refusal of the C entry points, (status, message) for (status, message): the case table of
tests/abi_refusal_cases.py against tests/golden/abi_refusals.json, which
tools/record_abi_refusals.py recorded from the library as it was before its entry points shared
their argument checks and table staging.  Which refusal wins when two apply is part of it (the
cases named "2: ...").  Python reads some of these messages (RTEngine.GUARD_MESSAGE, the tests
that match "tau layout only", "nothing was enqueued", ...), C callers may read any.

Nothing here is meant to reach a kernel except each entry point's one valid call; every status is
checked right after its call, so a wrongly accepted case ends the test before anything else
starts."""
import json
import os

import pytest

from tests import gpu_util as U

pytestmark = pytest.mark.gpu


def test_every_refusal_keeps_its_status_and_message():
    from rajepy_amd import _lib
    from rajepy_amd.engine import RTEngine
    from tests import abi_refusal_cases as T
    golden = json.load(open(os.path.join(U.GOLDEN, "abi_refusals.json")))
    assert set(golden) == set(T.ENTRIES)
    # every int-returning entry point with arguments beyond the context has its table
    takes_more = {n for n, (res, args) in _lib.SIGNATURES.items()
                  if res is _lib.C.c_int and len(args) > 1}
    assert takes_more == set(T.ENTRIES), takes_more ^ set(T.ENTRIES)
    eng = RTEngine(0)
    try:
        env = T.Env(eng)
        eng.synchronize()
        n = 0
        for name in T.ENTRIES:
            table = T.cases(name)
            assert {c for c, _ in table} == set(golden[name]), name
            for case, change in table:
                got = T.call(env, name, change)
                assert list(got) == golden[name][case], (name, case, got)
                n += 1
            assert T.call(env, name) == (_lib.RJP_OK, None), name
            eng.synchronize()
        assert eng.range_guard() is False
        print("\n%d refusals of %d entry points match the recorded ones" % (n, len(T.ENTRIES)))
    finally:
        eng.close()
