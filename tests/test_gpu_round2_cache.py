"""The queue kernel's round-2 cache (gcm_device.h, gcm_blocks_xN with R2C: the
open no-pack variants) at the only places it can go wrong, against the oracle.

The cache holds, per lane and record, four variants of the low counter byte's
part of the AES state after round 2 and, per four steps, the high byte's part
(tests/test_round2_cache_model.py states the map).  Its boundaries, in full
64-block steps of 1,024 bytes: 2 steps (one trip of the cached loop), the
first carry of lanes 62 and 63 at step 3 (4,096 B), the first reuse of a
variant under a new high byte at step 4 (6 steps), the second carry at step 7
(8,192 B), the longest TLS 1.2 record (16,384 B) and the TLS 1.3 padded limit
(16,640 B of ciphertext and tag).  An odd number of full steps leaves one for
the uncached tail after the cached loop; 4,080 / 4,112 and 8,176 put a partial
step after it, and two lengths are no multiple of 16.

The runner, fixtures and expectations are those of
test_gpu_record_handover.py (whole output buffer and every status compared,
sentinel-filled buffers, each batch twice) and, for a TLS 1.3 table, of
test_gpu_tls13.py.  Seal, the pack variants and the TLS 1.3 unit keep the
uncached code and run the same plans; the unhinted path selects the same
no-pack kernel on the device.
"""
import pytest

import test_gpu_record_handover as rh
import test_gpu_tls13 as g13
from test_gpu_record_handover import ta, engine, queue_impl  # noqa: F401  (fixtures)
from test_gpu_tls13 import aead, impl  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LENS = [2048, 3072, 4080, 4096, 4112, 5120, 6144, 8176, 8192, 16384, 7001, 12345]
# hints 3: fused no-pack kernel (the cached loop on open); 0: device-side selection
VARIANTS = [3, 0]


def _two_runs_plan():
    """A run of 40 records of session 0, then 40 of session 1, the lengths in
    turn (rotated in the second run).  The sequence numbers, so the nonces,
    differ from record to record."""
    plan = [(0, LENS[i % len(LENS)]) for i in range(40)]
    plan += [(1, LENS[(i + 5) % len(LENS)]) for i in range(40)]
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(rh.KINDS))
def test_two_runs_of_forty(ta, engine, oracle, queue_impl, name, mode, hints):
    """Every boundary length in two session runs; record 17 at an unaligned
    offset (it takes the other loop) and, on open, records 20 (8,192 B: both
    carries) and 44 (16,384 B) tampered: status -1, their plaintext
    zero-filled, the neighbours intact."""
    plan = _two_runs_plan()
    shifts = [0] * len(plan)
    shifts[17] = 5
    special = {20: rh.TAMPER, 44: rh.TAMPER} if mode == "open" else None
    rh._run_case(ta, engine, oracle, name, mode, hints, "r2c-two-runs", plan, special=special,
                 shifts=shifts)


def _second_records_plan():
    """8,448 records in runs of 40 over the five sessions: a workgroup's range
    is longer than its 16 waves (the engine gives a workgroup at least 16
    records and the GPU has 256 CUs), so waves take a second and a third record
    and a stale F or G of the previous record would show.  Neighbouring
    lengths differ in their number of steps, so in which variant and high byte
    the previous record ended."""
    lens = [2048, 4096, 3072, 8192, 5120, 2048, 6144, 4096, 4112, 16384, 2048, 4080, 3072]
    return [((i // 40) % rh.NSESS, lens[i % len(lens)]) for i in range(8448)]


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("name", list(rh.KINDS))
def test_second_and_third_record_of_a_wave(ta, engine, oracle, queue_impl, name, hints):
    rh._run_case(ta, engine, oracle, name, "open", hints, "r2c-second", _second_records_plan())


def _tls13_plan(mode):
    """Content lengths whose inner plaintext (content + type byte) has the
    lengths above and one byte more; on open also 16,384 bytes of content with
    239 of padding: 16,640 bytes of ciphertext and tag, the protocol's limit."""
    plan = []
    for run, sid in ((0, 0), (1, 1)):
        for i in range(40):
            n = LENS[(i + 5 * run) % len(LENS)]
            plan.append((sid, 21 + i % 3, n - (i % 2), 0, g13.GOOD))
    if mode == "open":
        plan[9] = (0, 23, 16384, 239, g13.GOOD)
        plan[49] = (1, 23, 16384, 239, g13.GOOD)
        plan[23] = plan[23][:4] + (g13.TAMPER,)
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(g13.KINDS))
def test_tls13_table(ta, engine, aead, impl, name, mode, hints):
    g13._run_case(ta, engine, aead, name, mode, hints, "r2c-" + mode, _tls13_plan(mode))
