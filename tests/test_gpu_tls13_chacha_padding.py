"""TLS 1.3 record padding on seal for TLSGPU_CHACHA20_POLY1305_TLS13 sessions:
the staged kernel's PAD instantiation against tests/tls13_padding.py over the
oracle's RFC 7905 AEAD.  Runner and conventions of test_gpu_tls13_padding.py
(sentinels, whole output image, every batch twice, 0xC3 around every content).

The staged kernel moves 16-byte pieces of 64-byte blocks in 128-byte steps, one
record per lane, so the content lengths sit around every piece, block and step
boundary (0, 1, 14-17, 47, 48, 62-65, 111, 112, 126-129, 255, 256) plus B - 1, B,
B + 1 of the session's block, with B = 0, 16, 64, 128, 512 and 16384 in one table:
about 700 records, not a multiple of 64.  Aligned and byte-shifted sources: the
aligned gather is the one that brings bytes past the content into the row.
"""
import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13
import tls13_padding as tp
import test_gpu_tls13_padding as gp

from test_gpu_tls13_padding import ta, engine, aead   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LENS = [0, 1, 14, 15, 16, 17, 47, 48, 62, 63, 64, 65, 111, 112, 126, 127, 128, 129, 255, 256]
BLOCKS = [0, 16, 64, 128, 512, 16384]
ORACLE_KIND = {5: po.CHACHA20_POLY1305}
GOLDEN = tp.GOLDEN_CHACHA_PADDED


def _lens(block):
    ls = set(LENS)
    if block > 1:
        ls |= {block - 1, block, block + 1}
    return sorted(n for n in ls if n <= 16384)


def _plan(sids, blocks):
    """700 records over the sessions `sids` (ChaCha sessions with padding blocks
    `blocks`): waves whose lanes alternate among the sessions, and whole waves of
    one session (the key words then come through the scalar path).  The B = 16384
    session gets 40 records (each is a 16 KiB output)."""
    plan, i = [], 0
    big = [s for s, b in zip(sids, blocks) if b == 16384]
    rest = [(s, b) for s, b in zip(sids, blocks) if b != 16384]
    while len(plan) < 448:                       # seven mixed waves
        s, b = rest[i % len(rest)]
        ls = _lens(b)
        plan.append((s, 21 + i % 3, ls[(i // len(rest) + i // 64) % len(ls)]))
        i += 1
    for w, (s, b) in enumerate(rest[1:4]):       # three whole waves of one padded session
        ls = _lens(b)
        plan += [(s, 21 + j % 3, ls[(j + 5 * w) % len(ls)]) for j in range(64)]
    for j in range(40):
        ls = _lens(16384)
        plan.append((big[0], 21 + j % 3, ls[j % len(ls)]))
    for j in range(20):                          # and a short last wave of all policies
        s, b = rest[j % len(rest)]
        plan.append((s, 22, _lens(b)[-1 - j % 3]))
    assert len(plan) == 700
    for s, b in zip(sids, blocks):
        assert {n for q, _, n in plan if q == s} >= set(_lens(b)), b
    return plan


def _shifts(layout, n):
    s = [0 if i % 2 == 0 else 1 + (i // 2) % 15 for i in range(n)]
    return (s if layout == "in-shifted" else None), (s if layout == "out-shifted" else None)


@pytest.mark.parametrize("layout", ["aligned", "in-shifted", "out-shifted"])
def test_padded_lengths_kind5_table(ta, engine, aead, layout):
    """A table of kind 5 only: the fused NARROW kernel, which checks the bounds
    itself.  The aligned case also opens the sealed image in place."""
    k5 = ta.CHACHA20_POLY1305_TLS13
    sessions = gp.make_sessions(ta, aead, [k5] * len(BLOCKS), BLOCKS, 21, ORACLE_KIND)
    plan = _plan(list(range(len(BLOCKS))), BLOCKS)
    ins, outs = _shifts(layout, len(plan))
    gp.run_seal(ta, engine, aead, sessions, ("cc-lengths",), plan, in_shifts=ins, out_shifts=outs,
                round_trip=layout == "aligned")


@pytest.mark.parametrize("layout", ["aligned", "in-shifted"])
def test_padded_lengths_beside_gcm(ta, engine, aead, layout):
    """Kind 5 beside padded AES-GCM sessions, hints 0: check_record_bounds, then
    the wide ChaCha kernel and the queue kernels on one batch."""
    k5 = ta.CHACHA20_POLY1305_TLS13
    kinds = [k5, ta.AES_128_GCM, k5, k5, ta.AES_256_GCM, k5, k5, k5]
    blocks = [0, 64, 16, 64, 512, 128, 512, 16384]
    sessions = gp.make_sessions(ta, aead, kinds, blocks, 22, ORACLE_KIND)
    cc = [i for i, k in enumerate(kinds) if k == k5]
    plan = _plan(cc, [blocks[i] for i in cc])
    plan += [(1 + 3 * (i % 2), 21 + i % 3, LENS[i % len(LENS)]) for i in range(90)]   # GCM records
    ins, outs = _shifts(layout, len(plan))
    gp.run_seal(ta, engine, aead, sessions, ("cc-mixed",), plan, hints=0, in_shifts=ins,
                out_shifts=outs, round_trip=layout == "aligned")


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("block,n", [(16, 20), (128, 1), (16384, 129)])
def test_output_bounds_use_the_padded_fragment(ta, engine, aead, mixed, block, n):
    """d_out ends where the last record's unpadded fragment would end."""
    k5 = ta.CHACHA20_POLY1305_TLS13
    kinds = [k5] * len(BLOCKS) + ([ta.AES_128_GCM] if mixed else [])
    blocks = BLOCKS + ([0] if mixed else [])
    sessions = gp.make_sessions(ta, aead, kinds, blocks, 23, ORACLE_KIND)
    plan = [(s % 5, 23, 30 + s) for s in range(150)] + [(BLOCKS.index(block), 22, n)]
    gp.run_seal(ta, engine, aead, sessions, ("cc-bounds", mixed, block, n), plan, cut_last=True)


def test_seal_wire_pads_each_fragment(ta, engine, aead):
    k5 = ta.CHACHA20_POLY1305_TLS13
    (p, ctx, block), = gp.make_sessions(ta, aead, [k5], [512], 24, ORACLE_KIND)
    table = ta.SessionTable(engine, 1)
    table.install(0, [p])
    rng = np.random.default_rng(10)
    jobs, seq = [], 1 << 32
    for frag in (0, 1000):
        for n in (1, 511, 512, 16383, 16384, 16385, 40000):
            data = rng.bytes(n)
            jobs.append((0, seq, 21 + len(jobs) % 3, data, frag,
                         tp.seal_wire(aead, ctx, p.fixed_iv, seq, 21 + len(jobs) % 3, data, block,
                                      frag)))
            seq += 100
    gp.run_seal_wire(ta, engine, table, k5, jobs, block)
    table.close()


def test_seal_wire_reproduces_the_padded_capture(ta, engine):
    """Every write of the TLS_CHACHA20_POLY1305_SHA256 connection captured under
    RecordPadding = 512, byte for byte, with the capture's keys."""
    fx = t13.load_fixture(GOLDEN)
    k5, block = ta.CHACHA20_POLY1305_TLS13, fx["record_padding"]
    dirs = fx["directions"]
    table = ta.SessionTable(engine, len(dirs))
    table.install(0, [ta.SessionParams(k5, d["key"], d["iv"], version=t13.VERSION, pad_block=block)
                      for d in dirs])
    gp.run_seal_wire(ta, engine, table, k5, gp.capture_jobs(fx), block)
    table.close()


def test_seal_host_spans(ta, engine, aead):
    k5 = ta.CHACHA20_POLY1305_TLS13
    sessions = gp.make_sessions(ta, aead, [k5] * len(BLOCKS), BLOCKS, 25, ORACLE_KIND)
    lens = [LENS[i % len(LENS)] for i in range(700)] + [16383, 16384, 1024, 1023, 511, 512] * 4
    gp.run_seal_host(ta, engine, aead, sessions, lens)
