"""The bits of fused attention against the recorded fixture tests/golden/attention_bits.json: every entry-point family
(plain, dropout, GAT, GAT with dropout) in fp32 and bf16, through every value of every template parameter of the
kernels, on one small pattern whose long rows take the chunk / combine path as well (tests/golden/
make_attention_bits.py has the cases and records the fixture).  The other attention suites compare with references,
several of them within a tolerance; this one holds out, stat and the four gradients to the recorded bits, so a
rounding that moves shows.  A change of the arithmetic on purpose records the fixture again and says so."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
spec = importlib.util.spec_from_file_location("make_attention_bits", GOLDEN / "make_attention_bits.py")
bits = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def recorded():
    return json.loads((GOLDEN / "attention_bits.json").read_text())


@pytest.fixture(scope="module")
def csr(recorded):
    rowptr, col = bits.pattern()
    assert {"rowptr": bits.sha(rowptr), "col": bits.sha(col)} == recorded["pattern"], \
        "the regenerated pattern differs from the recorded one: the inputs differ, not the kernels"
    return rowptr, col


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded["cases"]) == sorted(c["name"] for c in bits.cases())


@pytest.mark.parametrize("dtype", list(bits.DTYPES))
@pytest.mark.parametrize("family", ["attention", "gat"])
def test_bits(recorded, csr, family, dtype):
    rowptr, col = csr
    wrong = []
    for case in bits.cases():
        if case["family"] != family or case["dtype"] != dtype:
            continue
        want = recorded["cases"][case["name"]]
        ins, got = bits.run_case(case, rowptr, col)
        assert ins == want["inputs"], \
            f"{case['name']}: the regenerated inputs differ from the recorded ones " \
            f"({[n for n in ins if ins[n] != want['inputs'].get(n)]}): the inputs differ, not the kernels"
        assert sorted(got) == sorted(want["results"]), case["name"]
        wrong += [f"{case['name']}: {n}" for n in got if got[n] != want["results"][n]]
    assert not wrong, f"{len(wrong)} tensors differ from the recorded bits, the first of them: {wrong[:12]}"
