"""CPU suite: the size of every workspace and the refusal of a short one, against tests/golden/workspace_bytes.json
(recorded by tests/golden/make_workspace_golden.py before the layouts moved onto one function per workspace).

Each workspace has one layout function; its public psa_*_workspace_bytes is that function over a NULL base.  The
fixture pins what callers see of it: the bytes for arguments on both sides of every threshold, and that an entry
point handed one byte less than it asks for answers PSA_ERR_WORKSPACE with its own message before it touches
anything.  The cases and why a wrong acceptance is harmless: tests/workspace_cases.py."""
import json
from pathlib import Path

import pytest

import workspace_cases as wc

PSA_ERR_INVALID_ARG, PSA_ERR_WORKSPACE = 1, 3
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "workspace_bytes.json").read_text())


def size_functions():
    from paddle_sparse_amd import _lib

    return sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))


def test_every_size_function_is_recorded():
    """A size function added later cannot skip this suite: it needs a grid and a record."""
    names = size_functions()
    assert len(names) >= 22
    for name in names:
        assert name in wc.SIZE_GRIDS, f"{name}: add its argument grid to tests/workspace_cases.py"
        assert name in GOLDEN["sizes"], f"{name}: not in the fixture (tests/golden/make_workspace_golden.py)"
        assert [row[:-1] for row in GOLDEN["sizes"][name]] == wc.size_calls(name), f"{name}: fixture and grid differ"


@pytest.mark.parametrize("name", sorted(wc.SIZE_GRIDS))
def test_sizes_are_the_recorded_ones(name):
    from paddle_sparse_amd import _lib

    fn = getattr(_lib.load(), name)
    for *args, want in GOLDEN["sizes"][name]:
        assert fn(*args) == want, f"{name}{tuple(args)}"


def test_every_refusal_case_is_recorded():
    assert sorted(GOLDEN["refusals"]) == sorted(map(wc.case_id, wc.CASES))
    assert sorted(GOLDEN["misaligned"]) == sorted(map(wc.case_id, wc.MISALIGNED_CASES))


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_short_workspace_is_refused(case):
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    args, keep = wc.build_call(lib, case)
    status = getattr(lib, case[0])(*args)
    message = lib.psa_last_error().decode()
    assert (status, message) == (PSA_ERR_WORKSPACE, GOLDEN["refusals"][wc.case_id(case)])


@pytest.mark.parametrize("case", wc.MISALIGNED_CASES, ids=wc.case_id)
def test_misaligned_workspace_is_refused(case):
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    args, keep = wc.build_call(lib, case, misaligned=True)
    status = getattr(lib, case[0])(*args)
    message = lib.psa_last_error().decode()
    assert (status, message) == (PSA_ERR_INVALID_ARG, GOLDEN["misaligned"][wc.case_id(case)])
