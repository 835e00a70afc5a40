"""GPU (MI355X): every row of the per-conv kernels' launch table that a context can reach runs on the device at least once -- the fixed matrix of small calls of
tests/conv_rows_common.py (which rows each case reaches: tests/test_conv_table_cpu.py) -- and computes the bytes it computed before the launchers were
table-driven: logits and split modes of every case against tests/golden/conv_rows.npz, captured on an MI355X from the commit before with this same script
(twice, in two processes, equal bytes).

The dispatcher reads its switches once per process: each environment runs in ONE fresh child process (started, not exec'd), one at a time, each under its own
time limit; this process holds no GPU context of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_rows_common as crc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(crc.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("env", list(crc.ENVS))
def test_rows_compute_the_same_bytes(pkg, env, golden, tmp_path):
    pkg.build.build_lib()
    out = str(tmp_path / f"{env}.npz")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MLT_")}
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(crc.ROOT, "tests", "conv_rows_common.py"), "run", env, out],
                       env=dict(clean, **crc.ENVS[env]), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stderr[-3000:]}"
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    mine = [i for i, c in enumerate(crc.CASES) if c[0] == env]
    assert sorted(got) == sorted(f"c{i}_{what}" for i in mine for what in ("logits", "split", "arith"))
    for i in mine:
        _, size, n, tier, w2, x = crc.CASES[i]
        exact, w2_units, x_units = (int(v) for v in got[f"c{i}_arith"])
        # the context is in the state the case's plan was described for
        assert (w2_units, x_units) == (w2, x), f"case {crc.CASES[i]}: mlt_arithmetic reports w2_units {w2_units:#x} x_units {x_units:#x}"
        assert exact == (3 if w2 else 1 if tier in (1, 5) else 0), f"case {crc.CASES[i]}: arithmetic {exact}"
        assert got[f"c{i}_logits"].shape == (n, 9 if size == 128 else 15) and np.isfinite(got[f"c{i}_logits"]).all()
        for what in ("arith", "split", "logits"):
            g, w = got[f"c{i}_{what}"], golden[f"c{i}_{what}"]
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), \
                f"case {crc.CASES[i]}: {what} differ from the fixture" + (f", max |d| {np.abs(g - w).max():.3e}" if what == "logits" else "")
