"""bench.py --dump-outputs / --full: the sample a dump holds is fixed (no GPU),
and a plain run of a small config-B batch writes the last timed step's
statuses and sampled plaintexts, the same on every run, without the --full
extras in its result line (GPU)."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_dump", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_bounded():
    bench = _bench_module()
    n = 5000
    lengths = np.random.default_rng(7).integers(64, 16385, n)
    tampered = np.zeros(n, dtype=bool)
    tampered[512::1024] = True
    wl = types.SimpleNamespace(n=n, lengths=lengths, tampered=tampered)
    a, b = bench.dump_sample(wl, 1 << 20), bench.dump_sample(wl, 1 << 20)
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < n      # record order, no repeats
    assert int(lengths[a].sum()) <= 1 << 20
    assert set(np.nonzero(tampered)[0][:4]) <= set(a.tolist())      # the zero-filled path is in it
    # one more record would not fit: the budget is used, not a token sample
    assert int(lengths[a].sum()) + 16384 > 1 << 20
    # a budget smaller than any record still yields one record
    assert len(bench.dump_sample(wl, 1)) == 1
    # whole batch within the budget: every record
    small = types.SimpleNamespace(n=8, lengths=np.full(8, 100), tampered=np.zeros(8, dtype=bool))
    assert np.array_equal(bench.dump_sample(small, 1 << 20), np.arange(8))


def _run(tmp, name, *extra):
    out = os.path.join(tmp, name)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-ms", "0", "--records", "2048", "--dump-outputs", out, *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path):
    from talos_amd.workload import fill_bytes
    bench = _bench_module()
    line, d1 = _run(str(tmp_path), "a")
    _, d2 = _run(str(tmp_path), "b")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert "cpu_baseline" not in line                     # --full only
    assert sorted(os.listdir(d1)) == ["plaintext.npy", "status.npy"]
    st, pt = np.load(os.path.join(d1, "status.npy")), np.load(os.path.join(d1, "plaintext.npy"))
    assert st.dtype == np.float32 and pt.dtype == np.float32
    assert st.nbytes + pt.nbytes <= 64_000_000
    # config B's rule: 16 KiB records, records 512, 1536 (every 1024th from 512) tampered
    want = np.full(2048, 16384, dtype=np.float32)
    want[512::1024] = -1
    assert np.array_equal(st, want)
    tampered = want < 0
    wl = types.SimpleNamespace(n=2048, lengths=np.full(2048, 16384), tampered=tampered)
    idx = bench.dump_sample(wl, bench.DUMP_SAMPLE_BYTES)
    assert len(idx) == bench.DUMP_SAMPLE_BYTES // 16384 and pt.size == len(idx) * 16384
    rows = pt.reshape(len(idx), 16384)
    seed = bench.CONFIGS["B"][4]
    pos = {int(r): k for k, r in enumerate(idx)}
    assert not rows[pos[512]].any() and not rows[pos[1536]].any()    # tampered: zero-filled
    for r in (int(idx[0]), int(idx[len(idx) // 2]), int(idx[-1])):
        if not tampered[r]:
            exp = np.frombuffer(fill_bytes(seed, r, 16384), dtype=np.uint8).astype(np.float32)
            assert np.array_equal(rows[pos[r]], exp), r
    # same arguments, same inputs: a second run's outputs are equal array for array
    for f in ("status.npy", "plaintext.npy"):
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))), f
