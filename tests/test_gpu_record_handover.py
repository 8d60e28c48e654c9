"""The queue kernel's record hand-over and lengths-block table, against the oracle.

A wave of the queue kernel (gcm_hybrid.h) takes record after record from its
session run's queue; what it does between two records' step loops — the claim,
the descriptor and first loads of the next record, the finish of the previous
one (gcm_finish with the run's LEN * H table, gcm_device.h len_term) — is
shared by every record shape.  The shapes below are the ones at which that
code takes another path: 0 to 5 and 16 full 64-block steps with and without a
masked tail and a partial last block, aligned next to unaligned records, runs
that end inside a workgroup's range, and records the kernel skips (out of
bounds, publicly invalid, empty session) or zero-fills (tampered) directly
next to good ones.  Every output byte, tag and status is compared with the
oracle's tls1_enc, the output buffer and the status words start from a
sentinel, and each batch runs twice on fresh buffers.

Batches hold more than 16 records per workgroup (the engine gives one
workgroup per CU at least 16 records: above 4096 records a range is longer
than the workgroup's 16 waves), so waves do take a second record.

The helpers used here (RecordBatch, the oracle's TLS sessions) carry 16-byte
tags only, so no session with a shorter tag is included; test_gpu_tag_len.py
runs tag lengths 1..16 through the same kernel variants with batches it lays
out itself.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pyoracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM}
# 0..5 and 16 full steps (1024 B each), masked tails, partial last blocks
LENS = [0, 1, 16, 1008, 1024, 1040, 2032, 2048, 2064, 3072, 4096, 4112, 5120, 16384]
# hints 3: fused no-pack kernel; 0: device-side selection; 2: fused pack variant
VARIANTS = [3, 0, 2]
NSESS = 5           # installed sessions, different keys; session NSESS stays empty
SENTINEL = 0x5A5A5A5A
GOOD, TAMPER, OOB, INVALID, EMPTY = range(5)


@pytest.fixture(scope="module")
def ta():
    import talos_amd
    talos_amd.load_library()
    return talos_amd


@pytest.fixture(scope="module")
def engine(ta):
    e = ta.Engine(0)
    yield e
    e.close()


@pytest.fixture
def queue_impl(ta):
    prev = ta.get_gcm_impl()
    ta.set_gcm_impl("queue")
    yield
    ta.set_gcm_impl(prev)


_sealed = {}  # (name, plan key) -> (params, records, oracle bodies), computed once


def _material(ta, oracle, name, key, plan):
    """plan: [(session, plaintext length)].  The sessions' keys, the plaintext
    records and the oracle's sealed bodies, shared by the cases of one plan."""
    if (name, key) not in _sealed:
        kind = KINDS[name]
        rng = np.random.default_rng(len(plan) + 7 * kind)
        params = [ta.SessionParams(kind, rng.bytes(po.KEY_LEN[kind]), rng.bytes(4))
                  for _ in range(NSESS)]
        osess = [oracle.tls_session(p.aead, p.key, p.fixed_iv, p.version) for p in params]
        recs = [(sid, 1000 + i, 23, rng.bytes(n), kind) for i, (sid, n) in enumerate(plan)]
        bodies = [oracle.tls_seal(osess[sid], seq, rt, pt) for sid, seq, rt, pt, _ in recs]
        _sealed[(name, key)] = (params, recs, bodies)
    return _sealed[(name, key)]


def _run_case(ta, engine, oracle, name, mode, hints, key, plan, special=None, shifts=0):
    """Run the plan's records (seal: plaintext in, open: the oracle's bodies in)
    twice and compare the whole output buffer and every status with the image
    the oracle's results give.  special: {record index: TAMPER / OOB / INVALID /
    EMPTY}."""
    from talos_amd.batch import RecordBatch
    special = special or {}
    params, recs, bodies = _material(ta, oracle, name, key, plan)
    table = ta.SessionTable(engine, NSESS + 1)
    table.install(0, params)
    table.hint(hints)
    entries = []
    for i, ((sid, seq, rt, pt, kind), body) in enumerate(zip(recs, bodies)):
        what = special.get(i, GOOD)
        payload = pt if mode == "seal" else body
        if what == TAMPER:
            b = bytearray(payload)
            b[(7 * i) % len(b)] ^= 1 << (i % 8)
            payload = bytes(b)
        elif what == INVALID:
            payload = payload[:8 + 16 - 1 - i % 3]   # len < explicit nonce + tag
        entries.append((NSESS if what == EMPTY else sid, seq, rt, payload, kind))
    images = []
    for _ in range(2):
        batch = RecordBatch(engine, entries, mode, in_shift=shifts)
        descs = batch.d_recs.download().view(ta.RECORD_DTYPE).copy()
        for i, what in special.items():
            if what == OOB:
                descs[i]["in_off"] = batch.d_in.nbytes + 16   # past d_in even when empty
        batch.d_recs.upload(descs.view(np.uint8))
        batch.d_status.upload(np.full(max(batch.n, 1), SENTINEL, dtype=np.uint32).view(np.uint8))
        batch.run(table)
        engine.sync()
        out = batch.d_out.download().copy()
        st = batch.d_status.download().view(np.int32)[:batch.n].copy()
        images.append((out, st))
        exp_out = np.full(out.shape, 0xA5, dtype=np.uint8)
        exp_st = np.zeros(batch.n, dtype=np.int32)
        for i, ((sid, seq, rt, pt, kind), body) in enumerate(zip(recs, bodies)):
            what = special.get(i, GOOD)
            o = batch.out_offs[i]
            if what == OOB:
                exp_st[i] = ta.REC_OUT_OF_BOUNDS
            elif what in (INVALID, EMPTY):
                exp_st[i] = ta.REC_PUBLIC_INVALID
            elif what == TAMPER:
                exp_st[i] = ta.REC_BAD_MAC
                exp_out[o:o + len(pt)] = 0
            else:
                res = body if mode == "seal" else pt
                exp_st[i] = len(res)
                exp_out[o:o + len(res)] = np.frombuffer(res, dtype=np.uint8)
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (name, mode, hints, "status", bad[:8].tolist(), st[bad[:8]].tolist(),
                               exp_st[bad[:8]].tolist(), [plan[j] for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            offs = np.asarray(batch.out_offs)
            rec = int(np.searchsorted(offs, diff[0], side="right")) - 1
            raise AssertionError((name, mode, hints, "output byte", int(diff[0]), "record", rec,
                                  plan[rec], special.get(rec, GOOD)))
        batch.free()
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    table.close()


def _pairs_plan():
    """Every ordered pair of LENS as neighbours, one 392-record sequence per
    session run (rotated from run to run), 21 runs over the 5 sessions: 8232
    records, 33 per workgroup, so ranges end inside runs."""
    seq = [n for a in LENS for b in LENS for n in (a, b)]
    plan = []
    for run in range(21):
        rot = (37 * run) % len(seq)
        plan += [(run % NSESS, n) for n in seq[rot:] + seq[:rot]]
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_length_pairs(ta, engine, oracle, queue_impl, name, mode, hints):
    """Loop entry and exit: a record that runs the wide step loop next to one
    that skips it and the other way round, every ordered pair of lengths."""
    _run_case(ta, engine, oracle, name, mode, hints, "pairs", _pairs_plan())


def _runs_plan():
    """Session runs of 1, 2, 15, 16, 17, 33 and 64 records in turn, the five
    sessions in turn, all the lengths cyclically within every run: 6068 records,
    24 per workgroup, so a workgroup sees 1 to 5 sessions and ranges end inside
    runs."""
    plan, k = [], 0
    for c in range(41):
        for j, run_len in enumerate((1, 2, 15, 16, 17, 33, 64)):
            sid = (7 * c + j) % NSESS
            for _ in range(run_len):
                plan.append((sid, LENS[k % len(LENS)]))
                k += 1
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_run_boundaries_mixed_lengths_and_alignment(ta, engine, oracle, queue_impl, name, mode, hints):
    """Run boundaries (a claim must not cross a run or be taken twice: a wrong
    or unwritten status), mixed lengths in one run (every nibble position of the
    bit count in the LEN * H table) and 16-B aligned slots alternating with
    byte-aligned ones."""
    plan = _runs_plan()
    shifts = [0 if i % 2 == 0 else 1 + (i // 2) % 15 for i in range(len(plan))]
    _run_case(ta, engine, oracle, name, mode, hints, "runs", plan, shifts=shifts)


def _status_plan(mode):
    """Runs of 20 records (5120 records, 20 per workgroup): in every run one
    special record directly after and before a good one (position 3) and one as
    the run's last record; kinds and lengths rotate over the runs."""
    kinds = [OOB, EMPTY] + ([TAMPER, INVALID] if mode == "open" else [])
    plan, special = [], {}
    for run in range(256):
        for j in range(20):
            plan.append((run % NSESS, LENS[(run + 3 * j) % len(LENS)]))
        base = 20 * run
        special[base + 3] = kinds[run % len(kinds)]
        special[base + 19] = kinds[(run // len(kinds) + 1) % len(kinds)]
    for i, what in list(special.items()):
        if what == TAMPER and mode == "seal":
            del special[i]
    return plan, special


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_statuses_next_to_good_records(ta, engine, oracle, queue_impl, name, mode, hints):
    """Out-of-bounds, publicly invalid, empty-session and tampered records
    before, after and at the end of good records of the same run: exact
    statuses, zero-filled plaintext for BAD_MAC only, nothing else written."""
    plan, special = _status_plan(mode)
    _run_case(ta, engine, oracle, name, mode, hints, "status-" + mode, plan, special=special)


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_lengths_block_formula(ta, engine, oracle, queue_impl, name, mode, hints):
    """The lengths block as LEN * H from the table with lane nb % 64 at weight
    H^65: nb = 0, 1, 62, 63 (the AAD lane), 64, 65, 127, 128 and 1024 blocks,
    whole and with a partial last block."""
    plan = []
    for nb in (0, 1, 62, 63, 64, 65, 127, 128, 1024):
        plan.append((0, 16 * nb))
        if nb:
            plan.append((0, 16 * nb - 5))
    _run_case(ta, engine, oracle, name, mode, hints, "formula", plan)
