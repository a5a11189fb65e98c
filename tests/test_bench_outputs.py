"""bench.py --dump-outputs and the plain run: the dump keeps a fixed sample of rows inside its byte budget, in float32 /
float64 (CPU); a plain run prints the headline line only and dumps what its last step computed (GPU)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_dump_is_a_fixed_row_sample_inside_the_budget(tmp_path):
    import bench

    M, F = 300_000, 128
    out = torch.randn(M, F)
    arg = torch.randint(0, 1 << 40, (M, F))
    paths = bench.dump_outputs((out, arg), tmp_path, 1, 0)
    assert [p.name for p in paths] == ["out.npy", "arg_out.npy"]
    a, b = np.load(tmp_path / "out.npy"), np.load(tmp_path / "arg_out.npy")
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape and a.shape[1] == F
    assert a.nbytes + b.nbytes <= bench.DUMP_BYTES and a.shape[0] == bench.DUMP_BYTES // (12 * F)
    rows = np.sort(np.random.default_rng(0).choice(M, size=a.shape[0], replace=False))
    assert np.array_equal(a, out.numpy()[rows]) and np.array_equal(b, arg.numpy()[rows].astype(np.float64))
    # the same call again writes the same rows
    bench.dump_outputs((out, arg), tmp_path, 1, 0)
    assert np.array_equal(np.load(tmp_path / "out.npy"), a)


def test_dump_of_a_small_half_width_output_is_whole_and_per_rank(tmp_path):
    import bench

    out = torch.randn(1000, 16).to(torch.bfloat16)
    paths = bench.dump_outputs(out, tmp_path, 4, 3)
    assert [p.name for p in paths] == ["out_rank3.npy"]
    got = np.load(paths[0])
    assert got.dtype == np.float32 and np.array_equal(got, out.float().numpy())


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_below_one_are_refused_before_any_work(flags):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *flags], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr and p.stdout == ""


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs",
                        str(tmp_path / "dump")], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "spmm_sum_gedges_per_s" and line["unit"] == "GEdges/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["dtype"] == "f32" and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["full"] is False and not {"roofline", "cpu_baseline", "c3_other_ops", "power_law"} & set(line)
    assert sorted(f.name for f in (tmp_path / "dump").iterdir()) == ["out.npy"]
    got = np.load(tmp_path / "dump" / "out.npy")
    assert got.dtype == np.float32 and got.nbytes <= 64 << 20

    # the same seeded workload rebuilt here; the sampled rows summed in fp64 by torch (no HIP kernel involved)
    import bench

    dev = torch.device("cuda", 0)
    rowptr, col, val = bench.make_workload(bench.M_PER_GPU, bench.M_PER_GPU, bench.NNZ_PER_GPU, bench.FEAT, seed=2,
                                           device=dev)
    B = torch.randn(bench.M_PER_GPU, bench.FEAT, generator=torch.Generator(device=dev).manual_seed(100), device=dev)
    rows = np.sort(np.random.default_rng(0).choice(bench.M_PER_GPU, size=got.shape[0], replace=False))
    r = torch.from_numpy(rows).to(dev)
    lo, hi = rowptr[r], rowptr[r + 1]
    deg = hi - lo
    seg = torch.repeat_interleave(torch.arange(r.numel(), device=dev), deg)
    e = torch.arange(int(deg.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
    e = e + torch.repeat_interleave(lo, deg)
    terms = val[e].double()[:, None] * B[col[e]].double()
    ref = torch.zeros(r.numel(), bench.FEAT, dtype=torch.float64, device=dev).index_add_(0, seg, terms)
    scale = torch.zeros_like(ref).index_add_(0, seg, terms.abs())
    err = (torch.from_numpy(got).to(dev).double() - ref).abs()
    assert bool((err <= 1e-5 * scale + 1e-30).all())
