"""Record what every workspace costs and how a short one is refused: tests/golden/workspace_bytes.json, checked by
tests/test_workspace_layout.py.

    python tests/golden/make_workspace_golden.py          # no GPU needed; writes the fixture

"sizes": for every psa_*_workspace_bytes of the binding table, its value over the grid of tests/workspace_cases.py
(one list [arguments..., bytes] per call).  "refusals": for every case there, the message a workspace declared too
small is refused with (the status is always PSA_ERR_WORKSPACE); "misaligned": the same for a full-size workspace that is
not 16-byte aligned (PSA_ERR_INVALID_ARG).  Sizes, layouts and messages are part of the C-ABI: a
pull request that changes one on purpose runs this tool again and says so; one that reorganises the host code must
leave the fixture alone."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
FIXTURE = Path(__file__).resolve().parent / "workspace_bytes.json"
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main():
    import workspace_cases as wc
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    names = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    missing = [n for n in names if n not in wc.SIZE_GRIDS]
    if missing:
        raise SystemExit(f"no grid for {missing}; nothing recorded")
    sizes = {n: [args + [getattr(lib, n)(*args)] for args in wc.size_calls(n)] for n in names}
    refusals, misaligned = {}, {}
    for record, cases, how, want in ((refusals, wc.CASES, False, 3), (misaligned, wc.MISALIGNED_CASES, True, 1)):
        for case in cases:
            args, keep = wc.build_call(lib, case, misaligned=how)
            status = getattr(lib, case[0])(*args)
            if status != want:
                raise SystemExit(f"{wc.case_id(case)}: status {status}, not {want}; nothing recorded")
            record[wc.case_id(case)] = lib.psa_last_error().decode()
    lines = [f"{json.dumps(n)}: {json.dumps(rows)}" for n, rows in sizes.items()]  # a function per line
    FIXTURE.write_text('{"sizes": {\n' + ",\n".join(lines) + '\n},\n"refusals": ' +
                       json.dumps(refusals, indent=1, sort_keys=True) + ',\n"misaligned": ' +
                       json.dumps(misaligned, indent=1, sort_keys=True) + "}\n")
    json.loads(FIXTURE.read_text())
    print(f"{sum(map(len, sizes.values()))} sizes, {len(refusals)} refusals -> {FIXTURE}")


if __name__ == "__main__":
    main()
