"""The queue kernel's record finish with one GHASH reduction per multiply, and
the lengths-block table built with one shift and one fold, against the oracle.

The no-pack variants of the queue kernel weight each lane's chain with
mul_shoup_fold and every variant reads the LEN * H table that load_len_table
builds through gh_fold (gcm_device.h; the CPU model of both is
test_ghash_fold_model.py).  Built like test_gpu_record_handover.py: every
output byte, tag and status against the oracle's tls1_enc (TLS 1.3: the
oracle's AEAD under tests/tls13_helper.py), output and status buffers from a
sentinel, each batch twice.

Record lengths: block counts nb = 0, 1, 2, 62, 63, 64, 65, 127, 128, 129 and
1,024, whole and with a partial last block — lane l < nb weighs H^(nb + 1 - l')
with l' the lane's last block, so between them every weight 2..65 occurs (H^1
is the lengths block's, which the table carries; the pack variants multiply by
it in the lane of block nb), the H^65 lane nb % 64, the AAD-only lane 63
(nb <= 62) and empty chains — plus 1,
2, 30, 510, 8,190 and 16,384 bytes, whose bit counts put a non-zero nibble in
each row of the lengths table that a record can reach (rows 0..4).

Layout: the engine gives a workgroup at least 16 records and one workgroup
per CU, so a range is longer than the 16 waves only above 4,096 records; the
batch holds 24 per CU of a 256-CU device, in session runs of 17, 3 and 4
records over five sessions with different keys.  A workgroup's range thus
holds three runs (tables and lengths table rebuilt between them), and the
17-record run gives a wave its second record.  In open batches a tampered
record stands between good ones in every tenth run: BAD_MAC and zero-filled.
"""
import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13

pytestmark = pytest.mark.gpu

KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM}
NBS = [0, 1, 2, 62, 63, 64, 65, 127, 128, 129, 1024]
LENS = sorted({16 * nb for nb in NBS} | {16 * nb - 5 for nb in NBS if nb} |
              {1, 2, 30, 510, 8190, 16384})
VARIANTS = [3, 0, 2]    # fused no-pack, device-side selection, fused pack variant
NSESS = 5
RUNS = (17, 3, 4)
NREC = 24 * 256
SENTINEL = 0x5A5A5A5A


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


def _plan():
    """[(session, length)]: runs of 17, 3, 4, ... records, the sessions in
    turn, the lengths cyclically (31 lengths against a period of 24 records:
    every length meets every place in a run)."""
    plan, run = [], 0
    while len(plan) < NREC:
        for _ in range(RUNS[run % len(RUNS)]):
            plan.append((run % NSESS, LENS[len(plan) % len(LENS)]))
        run += 1
    return plan[:NREC]


def _tampered(plan):
    """One record in every tenth run, never the run's first or last."""
    out, start, run = set(), 0, 0
    for i in range(1, len(plan) + 1):
        if i == len(plan) or plan[i][0] != plan[i - 1][0]:
            if run % 10 == 0 and i - start >= 3:
                out.add(start + 1 + (run // 10) % (i - start - 2))
            start, run = i, run + 1
    return out


_cache = {}


def _material(ta, oracle, name, tls13):
    """Keys, plaintexts and the oracle's sealed records, once per key size and
    record generation.  TLS 1.3: `length` is the inner plaintext's (content
    and type byte; a zero length gives the type byte alone)."""
    if (name, tls13) not in _cache:
        kind = KINDS[name]
        plan = _plan()
        rng = np.random.default_rng(11 * kind + tls13)
        if tls13:
            params = [ta.SessionParams(kind, rng.bytes(po.KEY_LEN[kind]), rng.bytes(12),
                                       version=t13.VERSION) for _ in range(NSESS)]
            ctxs = [oracle.aead(p.aead, p.key) for p in params]
        else:
            params = [ta.SessionParams(kind, rng.bytes(po.KEY_LEN[kind]), rng.bytes(4))
                      for _ in range(NSESS)]
            ctxs = [oracle.tls_session(p.aead, p.key, p.fixed_iv, p.version) for p in params]
        recs = []
        for i, (sid, n) in enumerate(plan):
            seq = (1 << 33) + 1000 + i
            if tls13:
                content = rng.bytes(max(n - 1, 0))
                plain = t13.inner_plaintext(content, 23, 0)
                sealed = t13.seal_inner(oracle, ctxs[sid], params[sid].fixed_iv, seq, plain)
            else:
                content = plain = rng.bytes(n)
                sealed = oracle.tls_seal(ctxs[sid], seq, 23, plain)
                st, back = oracle.tls_open(ctxs[sid], seq, 23, sealed)
                assert st == 1 and bytes(back[:n]) == plain
            recs.append(dict(sid=sid, seq=seq, content=content, plain=plain, sealed=sealed))
        _cache[(name, tls13)] = (params, recs, _tampered(plan))
    return _cache[(name, tls13)]


def _run_case(ta, engine, oracle, name, mode, hints, tls13):
    from talos_amd.batch import RecordBatch
    params, recs, tampered = _material(ta, oracle, name, tls13)
    kind = KINDS[name]
    if mode == "seal":
        tampered = set()
    table = ta.SessionTable(engine, NSESS)
    table.install(0, params)
    table.hint(hints)
    entries = []
    for i, r in enumerate(recs):
        payload = r["content"] if mode == "seal" else r["sealed"]
        if i in tampered:
            b = bytearray(payload)
            b[(7 * i) % len(b)] ^= 1 << (i % 8)
            payload = bytes(b)
        entries.append((r["sid"], r["seq"], 23, payload, kind))
    images = []
    for _ in range(2):
        batch = RecordBatch(engine, entries, mode, tls13=True) if tls13 else \
            RecordBatch(engine, entries, mode)
        batch.d_status.upload(np.full(batch.n, SENTINEL, dtype=np.uint32).view(np.uint8))
        batch.run(table)
        engine.sync()
        out = batch.d_out.download().copy()
        st = batch.d_status.download().view(np.int32)[:batch.n].copy()
        images.append((out, st))
        exp_out = np.full(out.shape, 0xA5, dtype=np.uint8)
        exp_st = np.zeros(batch.n, dtype=np.int32)
        for i, r in enumerate(recs):
            o = batch.out_offs[i]
            if i in tampered:
                exp_st[i] = ta.REC_BAD_MAC
                exp_out[o:o + len(r["plain"])] = 0
                continue
            res = r["sealed"] if mode == "seal" else r["plain"]
            exp_st[i] = len(res) if mode == "seal" or not tls13 else len(r["content"])
            exp_out[o:o + len(res)] = np.frombuffer(res, dtype=np.uint8)
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (name, mode, hints, tls13, "status", bad[:8].tolist(),
                               st[bad[:8]].tolist(), exp_st[bad[:8]].tolist(),
                               [len(recs[j]["plain"]) for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            rec = int(np.searchsorted(np.asarray(batch.out_offs), diff[0], side="right")) - 1
            raise AssertionError((name, mode, hints, tls13, "output byte", int(diff[0]), "record",
                                  rec, len(recs[rec]["plain"]), rec in tampered))
        batch.free()
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    table.close()


def test_plan_covers_every_weight_and_table_row():
    """What the docstring claims of LENS (no GPU work: the plan alone)."""
    weights, rows = set(), set()
    for n in LENS:
        nb = (n + 15) >> 4
        for lane in range(64):
            if lane == nb % 64:
                weights.add(65)
            elif lane < nb:
                weights.add(nb + 1 - (lane + ((nb - 1 - lane) & ~63)))
            elif lane == 63:
                weights.add(nb + 2)
            else:
                weights.add(0)
        rows |= {p for p in range(6) if ((8 * n) >> (4 * p)) & 0xF}
    # weight 1 is the lengths block's: the table carries it (in the pack variants
    # the lane of block j = nb multiplies by H^1, mul_shoup)
    assert weights == {0} | set(range(2, 66))
    # row 5 holds bit counts from 2^20, past the record limit: never non-zero
    assert rows == set(range(5))
    plan = _plan()
    assert len(plan) > 16 * 256 and len(_tampered(plan)) > 20
    assert {s for s, _ in plan} == set(range(NSESS))


@pytest.mark.parametrize("tls13", [False, True], ids=["tls12", "tls13"])
@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_finish_and_lengths_table(ta, engine, oracle, queue_impl, name, mode, hints, tls13):
    _run_case(ta, engine, oracle, name, mode, hints, tls13)
