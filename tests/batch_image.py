"""Whole-image runs of tlsgpu_seal_batch / tlsgpu_open_batch for the tests that lay
their batches out themselves (test_gpu_tag_len.py, test_gpu_record_limit.py),
and the TLS 1.2 session model they share: pyoracle's generic framing
(tls_seal_record / tls_open_record) over the oracle's AEAD at the session's tag
length.  The engine's statuses are mapped here from tls1_enc's 1 / 0 / -1.

Conventions (those of test_gpu_tls13_padding.py::run_seal): slot i sits at a
16-byte boundary plus its shift, slots are 3 bytes apart, d_in is 0xC3 and d_out
0xA5 around every record, the status words start from a sentinel, the whole
output buffer and every status are compared with the model's image, every batch
runs twice on refilled buffers, and both device buffers are allocated 64 bytes
beyond the in_bytes / out_bytes the call is given; that slack must come back
untouched.  in_bytes ends at the last record's last input byte and out_bytes at
the last record's last output byte (`cut` bytes earlier: that record is then
TLSGPU_REC_OUT_OF_BOUNDS and not a byte of it is written).
"""
from dataclasses import dataclass

import numpy as np

import pyoracle as po

SENTINEL = 0x5A5A5A5A
SLACK = 64
GCM = (po.AES_128_GCM, po.AES_256_GCM)


@dataclass
class Session:
    kind: int
    params: object      # talos_amd.SessionParams
    ctx: object         # the oracle's AEAD at the session's tag length
    ctx16: object       # ... and with the full tag (what follows a truncated tag "on the wire")
    t: int              # effective tag length (tag_len 0 is 16)
    eiv: int            # explicit nonce bytes in the fragment


@dataclass
class Entry:
    """One record of a batch: what goes in, and what the model says comes out."""
    sid: int
    seq: int
    rtype: int
    inp: bytes          # seal: the plaintext; open: the fragment
    st: int             # expected status
    out: bytes          # expected bytes at out_off (b"": nothing is written)
    eiv: int = 0
    bait: bytes = b""   # bytes behind inp in d_in, outside the record's length
    reserve: int = 0    # bytes behind out that must stay free of the next slot


def make_sessions(ta, oracle, kinds, tags, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k, tag in zip(kinds, tags):
        p = ta.SessionParams(k, rng.bytes(po.KEY_LEN[k]), rng.bytes(po.FIXED_IV_LEN[k]), tag_len=tag)
        out.append(Session(k, p, oracle.aead(k, p.key, tag), oracle.aead(k, p.key, 16), tag or 16,
                           8 if k in GCM else 0))
    return out


def model_seal(oracle, s, seq, rtype, pt, full=False):
    return po.tls_seal_record(oracle, s.ctx16 if full else s.ctx, s.kind, s.params.fixed_iv, seq,
                              rtype, pt)


def seal_entry(ta, oracle, sessions, sid, seq, rtype, pt):
    s = sessions[sid]
    frag = model_seal(oracle, s, seq, rtype, pt)
    assert len(frag) == s.eiv + len(pt) + s.t
    return Entry(sid, seq, rtype, pt, len(frag), frag, s.eiv, reserve=16 - s.t)


def open_entry(ta, oracle, sessions, sid, seq, rtype, frag, bait=b""):
    """The model's verdict on `frag`, in the engine's terms."""
    s = sessions[sid]
    r, out = po.tls_open_record(oracle, s.ctx, s.kind, s.params.fixed_iv, seq, rtype, frag,
                                tag_len=s.t)
    if r == 0:
        return Entry(sid, seq, rtype, frag, ta.REC_PUBLIC_INVALID, b"", s.eiv, bait)
    n = len(frag) - s.eiv - s.t
    assert len(out) == n
    if r == 1:
        return Entry(sid, seq, rtype, frag, n, out, s.eiv, bait)
    assert r == -1 and out == bytes(n)
    return Entry(sid, seq, rtype, frag, ta.REC_BAD_MAC, out, s.eiv, bait)


def run_image(ta, engine, table, entries, seal, in_shifts=None, out_shifts=None, in_place=False,
              cut=0, label=None):
    """Lay `entries` out, run them twice and compare everything (module docstring)."""
    n = len(entries)
    assert n and len(entries[-1].out) > cut and not (in_place and (cut or seal))
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    ip = op = 0
    for i, e in enumerate(entries):
        ip += (-ip) % 16 + (in_shifts[i] if in_shifts else 0)
        if in_place:
            oo = ip + e.eiv
        else:
            op += (-op) % 16 + (out_shifts[i] if out_shifts else 0)
            oo = op
        descs[i] = (ip, oo, e.seq, e.sid, ta.len_type(len(e.inp), e.rtype))
        ip += len(e.inp) + len(e.bait) + 3
        op = oo + len(e.out) + max(3, e.reserve)
    in_offs = [int(d["in_off"]) for d in descs]
    out_offs = [int(d["out_off"]) for d in descs]
    in_bytes = in_offs[-1] + len(entries[-1].inp)
    out_bytes = in_bytes if in_place else out_offs[-1] + len(entries[-1].out) - cut
    host_in = np.full(in_bytes + SLACK, 0xC3, dtype=np.uint8)
    for o, e in zip(in_offs, entries):
        both = e.inp + e.bait
        host_in[o:o + len(both)] = np.frombuffer(both, dtype=np.uint8)
    exp_out = host_in.copy() if in_place else np.full(out_bytes + SLACK, 0xA5, dtype=np.uint8)
    exp_st = np.zeros(n, dtype=np.int32)
    for i, (o, e) in enumerate(zip(out_offs, entries)):
        if o + len(e.out) > out_bytes:
            assert cut and i == n - 1
            exp_st[i] = ta.REC_OUT_OF_BOUNDS              # and not a byte written
        else:
            exp_st[i] = e.st
            exp_out[o:o + len(e.out)] = np.frombuffer(e.out, dtype=np.uint8)
    d_in = ta.DeviceBuffer(engine, host_in.nbytes)
    d_out = d_in if in_place else ta.DeviceBuffer(engine, exp_out.nbytes)
    d_recs, d_status = ta.DeviceBuffer(engine, descs.nbytes), ta.DeviceBuffer(engine, 4 * n)
    d_recs.upload(descs.view(np.uint8))
    run = ta.seal_batch if seal else ta.open_batch
    images = []
    for _ in range(2):
        d_in.upload(host_in)
        if not in_place:
            d_out.fill(0xA5)
        d_status.upload(np.full(n, SENTINEL, dtype=np.uint32).view(np.uint8))
        run(table, d_recs.ptr, n, d_in.ptr, in_bytes, d_out.ptr, out_bytes, d_status.ptr, None)
        engine.sync()
        out = d_out.download().copy()
        st = d_status.download().view(np.int32)[:n].copy()
        images.append((out, st))
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (label, "status", bad[:8].tolist(), st[bad[:8]].tolist(),
                               exp_st[bad[:8]].tolist(),
                               [(entries[j].sid, len(entries[j].inp)) for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            at = int(diff[0])
            rec = max(int(np.searchsorted(np.asarray(out_offs), at, side="right")) - 1, 0)
            raise AssertionError((label, "output byte", at, "slack" if at >= out_bytes else "record",
                                  rec, "session", entries[rec].sid, "input length",
                                  len(entries[rec].inp), "at", at - out_offs[rec], "got",
                                  int(out[at]), "expected", int(exp_out[at]), "differing bytes",
                                  int(diff.size)))
        if not in_place:
            assert (d_in.download() == host_in).all(), (label, "d_in changed")
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    for b in {d_in, d_out, d_recs, d_status}:
        b.free()
