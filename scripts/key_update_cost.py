#!/usr/bin/env python3
"""What a device rekey costs: device-event time around
tlsgpu_sessions_key_update alone, for 1, 1,024 and 16,384 sessions of each TLS 1.3
suite, `--warmup` calls then the median of `--steps`; beside it the wall time of
tlsgpu_sessions_install for the same counts (the floor of the host route: that
route also needs a read-back and a host HKDF).  One JSON line per suite and count.

    python scripts/key_update_cost.py [--steps 10] [--warmup 3] [--install-only]

--install-only times the installs alone and uses nothing a build without the
key schedule lacks (TALOS_ROOT selects the tree whose package and library run).
Under `rocprofv3 --kernel-trace --stats -- python scripts/key_update_cost.py
--counts 16384` the stats split a rekey into tg::tls13_derive_kernel and
tg::tls13_install_kernel.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.environ.get("TALOS_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import talos_amd as ta  # noqa: E402

SUITES = {"aes128": (ta.AES_128_GCM, 32, 16), "aes256": (ta.AES_256_GCM, 48, 32),
          "chacha": (ta.CHACHA20_POLY1305_TLS13, 32, 32)}


def median_spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--counts", default="1,1024,16384")
    ap.add_argument("--install-only", action="store_true")
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    engine = ta.Engine(0)
    rng = np.random.default_rng(7)
    for suite, (kind, hashlen, key_len) in SUITES.items():
        for n in counts:
            table = ta.SessionTable(engine, n)
            out = dict(suite=suite, sessions=n)
            # the host route's floor: tlsgpu_sessions_install, wall time (it synchronises)
            params = [ta.SessionParams(kind, rng.bytes(key_len), rng.bytes(12), version=0x0304)
                      for _ in range(n)]
            arr = (ta._SessionParams * n)(*[p.to_c() for p in params])
            wall = []
            for k in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                rc = table.lib.tlsgpu_sessions_install(table.handle, 0, n, arr)
                t1 = time.perf_counter()
                assert rc == 0
                if k >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
            out["install_wall_ms"] = median_spread(wall)
            if not a.install_only:
                table.install_secrets(0, [ta.SecretParams(kind, rng.bytes(hashlen))
                                          for _ in range(n)])
                d_ids, d_st = ta.DeviceBuffer(engine, 4 * n), ta.DeviceBuffer(engine, 4 * n)
                d_ids.upload(np.arange(n, dtype=np.uint32).view(np.uint8))
                ms = []
                for k in range(a.warmup + a.steps):
                    e0, e1 = ta.Event(engine), ta.Event(engine)
                    e0.record()
                    table.key_update(d_ids.ptr, n, d_st.ptr)
                    e1.record()
                    engine.sync()
                    if k >= a.warmup:
                        ms.append(e0.elapsed_ms(e1))
                    e0.close()
                    e1.close()
                assert not d_st.download().view(np.int32).any()
                out["key_update_event_ms"] = median_spread(ms)
                d_ids.free()
                d_st.free()
            table.close()
            print(json.dumps(out), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
