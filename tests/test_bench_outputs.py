"""bench.py --dump-outputs / --full on CPU: the dump's formats, its size bound and its fixed
sample; what a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_formats_and_fixed_sample(tmp_path):
    """bytes are written whole as float32 and offsets as float64 while they fit; a larger array
    is cut to DUMP_ARRAY_BYTES at the same sorted indices in every call"""
    import torch
    import bench
    small = torch.arange(1000, dtype=torch.int64).to(torch.uint8)
    off = torch.arange(5, dtype=torch.int64) * (1 << 40) + 1  # not exact in float32
    keep = bench.DUMP_ARRAY_BYTES // 4
    big = (torch.arange(keep + 12345, dtype=torch.int64) * 7 % 251).to(torch.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "off": off, "big": big})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "off", "big")}
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], small.numpy())
    assert a["off"].dtype == np.float64 and np.array_equal(a["off"].astype(np.int64), off.numpy())
    assert a["big"].dtype == np.float32 and a["big"].shape == (keep,)
    assert os.path.getsize(tmp_path / "a" / "big.npy") <= bench.DUMP_ARRAY_BYTES + 128
    idx = np.sort(np.random.default_rng(bench.SEED).integers(0, big.numel(), size=keep))
    assert np.array_equal(a["big"], big.numpy()[idx])
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))


def test_plain_run_refuses_extras():
    """--e2e is one of the --full measurements: without --full it is an error, not a silent skip;
    a plain line still carries the headline fields"""
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--stub",  # noqa: E731
                                     "--steps", "2", "--warmup", "0", *a], capture_output=True,
                                    text=True, timeout=300, cwd=REPO)
    p = run("--e2e")
    assert p.returncode == 2 and "--full" in p.stderr
    for extra in ((), ("--full",)):
        p = run(*extra)
        assert p.returncode == 0, p.stderr
        out = json.loads(p.stdout.strip().splitlines()[-1])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in out
        assert out["steps"] == 2
