"""bench.py --dump-outputs: what the last timed step of the headline workload returned (the stacked image, or a fixed seeded
sample of it, and the clip counters), so that two builds can be compared output for output on identical inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    b = _bench_module()
    small = b.dump_sample_index(1000)
    assert np.array_equal(small, np.arange(1000))
    big = 4096 * 4096
    idx = b.dump_sample_index(big)
    assert idx.size == b.DUMP_MAX_PIXELS and idx.size * 4 <= 64 * 2 ** 20
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < big
    assert np.array_equal(idx, b.dump_sample_index(big))               # the same pixels on every run
    image = np.arange(big, dtype=np.float32)
    b.write_outputs(str(tmp_path), image, [3, 4])
    res = np.load(os.path.join(str(tmp_path), "result.npy"))
    assert res.dtype == np.float32 and np.array_equal(res, image[idx])
    cc = np.load(os.path.join(str(tmp_path), "clip_counters.npy"))
    assert cc.dtype == np.float64 and cc.tolist() == [3.0, 4.0]


def test_full_is_off_by_default_and_apply_needs_it(monkeypatch, capsys):
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "5"])
    assert b.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--apply"])
    assert b.parse().full is True
    monkeypatch.setattr(sys, "argv", ["bench.py", "--apply"])
    with pytest.raises(SystemExit):
        b.parse()
    assert "--full" in capsys.readouterr().err


def _bench(extra, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--frames", "16", "--width", "256", "--height", "96",
           "--steps", "3", "--warmup", "1", "--preheat-steps", "1", "--no-cpu", "--no-also",
           "--dump-outputs", out_dir] + extra
    p = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True,
                       timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    doc = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    return doc, np.load(os.path.join(out_dir, "result.npy")), np.load(os.path.join(out_dir, "clip_counters.npy"))


@pytest.mark.gpu
def test_dump_holds_what_the_timed_pass_returned(nl, tmp_path):
    one, res1, cc1 = _bench([], str(tmp_path / "one"))
    assert one["steps"] == 3 and one["roofline"]["timed_passes_averaged"] == 3 and one["ms_per_step"] > 0
    # a plain run measures the headline only: every other leg is --full's
    assert not {"ms_per_step_synchronous", "cpu_baseline", "fresh_handle", "apply_from_host", "also"} & set(one)
    # the same synthetic stack through the C ABI in this process
    with nl.StackHandle(16, 256, 96) as st:
        st.fill_synthetic()
        want, cl, ch = st.run(2, 3.0, 3.0)
    assert res1.dtype == np.float32 and res1.shape == want.shape
    assert cc1.tolist() == [cl, ch] == [one["config"]["clip_low"], one["config"]["clip_high"]]
    # two ranks (gloo, both on device 0): their tiles gathered into the same image
    two, res2, cc2 = _bench(["--gpus", "2", "--backend", "gloo", "--share-device"], str(tmp_path / "two"))
    assert two["n_gpus"] == 2 and cc2.tolist() == [cl, ch]
    ok = ~np.isnan(want)
    for res in (res1, res2):          # (sigma clipping: the register-resident kernels agree within the north star's 1e-5)
        assert np.array_equal(np.isnan(res), np.isnan(want))
        assert np.all(np.abs(res[ok].astype(np.float64) - want[ok]) <= 1e-5 * np.abs(want[ok]))
