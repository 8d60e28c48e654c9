#!/usr/bin/env python3
"""What TLS 1.3 record protection costs next to TLS 1.2 on the same build and
box: a B-shaped batch (64 Ki x 16 KiB records, 1,024 sessions, AES-128-GCM), a
D-shaped one (256 Ki records, Zipf lengths 64..16384, 1,024 sessions,
AES-256-GCM) and a C-shaped one (1 Mi x 1,400-byte records, 4,096 sessions,
ChaCha20-Poly1305: kind 3 / 0x0303 against kind 5 / 0x0304), sealed and opened
as TLS 1.2 and as TLS 1.3 sessions with the same keys, contents and sequence
numbers.  Timed between events on the engine
stream as bench.py does (warm-up launches, then `steps` launches between two
events); prints one JSON line per (shape, generation, op) and the ratios.

    python scripts/tls13_cost.py [--shape B|C|D|BD|...] [--gen 12|13|both] [--steps K] [--warmup W]

--pad B (TLS 1.3 seals only): what record padding costs.  Each shape is sealed
twice in the same process: by sessions with pad_block = B, and by sessions
without padding whose records have the content length of the padded ones
(inner - 1), so both write the same number of bytes; the difference is the
price of the padding blocks taking the kernels' tail paths.

Under `rocprofv3 --kernel-trace --stats -- python scripts/tls13_cost.py --gen 13
--steps 3` the stats list tg::tls13_unpad_kernel, the unpad pass's own time
(--shape C: the ChaCha sessions' pass).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import talos_amd as ta  # noqa: E402
from talos_amd.workload import KEY_TAG, IV_TAG, fill_bytes, zipf_lengths  # noqa: E402

SHAPES = {"B": (ta.AES_128_GCM, 65536, 1024, None, 0x5EED0001),
          "D": (ta.AES_256_GCM, 1 << 18, 1024, "zipf", 0x5EED0003),
          "C": (ta.CHACHA20_POLY1305, 1 << 20, 4096, 1400, 0x5EED0002)}
GIB = float(1 << 30)


def run(engine, shape, gen, steps, warmup, pad=0, as_padded=0):
    """pad: the sessions' pad_block; as_padded: no padding, but every record as
    long as pad_block = as_padded would make it (both: TLS 1.3, seal only)."""
    kind, n, nsess, dist, seed = SHAPES[shape]
    t13 = gen == 13
    lens = (np.full(n, 16384, dtype=np.int64) if dist is None
            else zipf_lengths(n, seed) if dist == "zipf" else np.full(n, dist, dtype=np.int64))
    inner_of = np.vectorize(ta.tls13_inner_len)
    if as_padded:
        lens = inner_of(lens, as_padded).astype(np.int64) - 1
    chacha = kind == ta.CHACHA20_POLY1305
    if chacha and t13:
        kind = ta.CHACHA20_POLY1305_TLS13     # the same cipher, key and 12-byte IV
    eiv, extra = (0, 1) if t13 else (0 if chacha else 8, 0)
    if pad:
        extra = inner_of(lens, pad).astype(np.int64) - lens      # type byte + padding, per record
    params = [ta.SessionParams(kind, fill_bytes(seed ^ KEY_TAG, s, ta.KEY_LEN[kind]),
                               fill_bytes(seed ^ IV_TAG, s, 12 if t13 or chacha else 4),
                               version=0x0304 if t13 else 0x0303, pad_block=pad)
              for s in range(nsess)]
    table = ta.SessionTable(engine, nsess)
    table.install(0, params)
    session = (np.arange(n) // (n // nsess)).astype(np.uint32)
    seq = (np.arange(n) % (n // nsess)).astype(np.uint64) + np.uint64(1 << 20)
    pt_slot = (lens + 15) // 16 * 16
    body_slot = (lens + eiv + extra + 16 + 15 + 16) // 16 * 16
    pt_off = np.concatenate([[0], np.cumsum(pt_slot)[:-1]]).astype(np.uint64)
    body_off = (np.concatenate([[0], np.cumsum(body_slot)[:-1]]) + (16 - eiv) % 16).astype(np.uint64)
    pt_bytes, body_bytes = int(pt_slot.sum()) + 16, int(body_slot.sum()) + 32
    # the open's output slots leave room for a TLS 1.3 record's inner type byte
    out_slot = (lens + extra + 15) // 16 * 16
    out_off = np.concatenate([[0], np.cumsum(out_slot)[:-1]]).astype(np.uint64)
    d_pt, d_body, d_out = (ta.DeviceBuffer(engine, b)
                           for b in (pt_bytes, body_bytes, int(out_slot.sum()) + 16))
    d_status = ta.DeviceBuffer(engine, 4 * n)
    d_offs, d_lens = ta.DeviceBuffer(engine, 8 * n), ta.DeviceBuffer(engine, 4 * n)
    d_offs.upload(pt_off.view(np.uint8))
    d_lens.upload(lens.astype(np.uint32).view(np.uint8))
    engine.fill_synthetic_spans(d_pt.ptr, d_offs.ptr, d_lens.ptr, n, seed)
    engine.sync()
    seal = np.zeros(n, dtype=ta.RECORD_DTYPE)
    seal["in_off"], seal["out_off"], seal["seq"], seal["session"] = pt_off, body_off, seq, session
    seal["len_type"] = (23 << 24) | lens.astype(np.uint32)
    frag = (lens + eiv + extra + 16).astype(np.uint32)
    opn = np.zeros(n, dtype=ta.RECORD_DTYPE)
    opn["in_off"], opn["out_off"], opn["seq"], opn["session"] = body_off, out_off, seq, session
    opn["len_type"] = (23 << 24) | frag
    d_seal, d_open = ta.DeviceBuffer(engine, seal.nbytes), ta.DeviceBuffer(engine, opn.nbytes)
    d_seal.upload(seal.view(np.uint8))
    d_open.upload(opn.view(np.uint8))
    results = {}
    for op, descs, lengths, d_i, d_o, want in (
            ("seal", d_seal, lens, d_pt, d_body, frag.astype(np.int32)),
            ("open", d_open, frag, d_body, d_out, lens.astype(np.int32))):
        if (pad or as_padded) and op == "open":
            continue
        table.hint(ta.batch_hints(lengths, session, op == "seal", tls13=t13,
                                  pad_blocks={s: pad for s in range(nsess)} if pad else None))
        fn = ta.seal_batch if op == "seal" else ta.open_batch

        def launch():
            fn(table, descs.ptr, n, d_i.ptr, d_i.nbytes, d_o.ptr, d_o.nbytes, d_status.ptr)
        for _ in range(warmup):
            launch()
        engine.sync()
        st = d_status.download().view(np.int32)[:n]
        if not np.array_equal(st, want):
            raise RuntimeError(f"{shape} gen {gen} {op}: {int((st != want).sum())} wrong statuses")
        e0, e1 = ta.Event(engine), ta.Event(engine)
        e0.record()
        for _ in range(steps):
            launch()
        e1.record()
        ms = e0.elapsed_ms(e1) / steps
        e0.close()
        e1.close()
        results[op] = ms
        print(json.dumps({"shape": shape, "tls": "1.3" if t13 else "1.2", "op": op, "records": n,
                          **({"pad_block": pad} if pad else {}),
                          **({"lengths_as_padded_to": as_padded} if as_padded else {}),
                          "wire_bytes": int(frag.astype(np.int64).sum()),
                          "payload_bytes": int(lens.sum()), "ms_per_launch": round(ms, 4),
                          "GiBps": round(float(lens.sum()) / (ms / 1e3) / GIB, 2),
                          "steps": steps, "warmup": warmup}), flush=True)
    if t13 and "open" in results:   # spot check: the opened content and inner type of a few records
        for i in (0, n // 2, n - 1):
            got = d_out.download(int(lens[i]) + 1, int(out_off[i]))
            ref = d_pt.download(int(lens[i]), int(pt_off[i]))
            assert np.array_equal(got[:-1], ref) and got[-1] == 23, i
    for b in (d_pt, d_body, d_out, d_status, d_offs, d_lens, d_seal, d_open):
        b.free()
    table.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="BD")
    ap.add_argument("--gen", default="both", choices=["12", "13", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pad", type=int, default=0, metavar="B",
                    help="TLS 1.3 seals with pad_block = B against unpadded records of the padded lengths")
    a = ap.parse_args()
    ta.load_library()
    engine = ta.Engine(0)
    for shape in a.shape if a.pad else "":
        padded = run(engine, shape, 13, a.steps, a.warmup, pad=a.pad)["seal"]
        plain = run(engine, shape, 13, a.steps, a.warmup, as_padded=a.pad)["seal"]
        print(json.dumps({"shape": shape, "pad_block": a.pad,
                          "padded_over_unpadded_same_lengths_time": round(padded / plain, 4)}),
              flush=True)
    for shape in "" if a.pad else a.shape:
        res = {g: run(engine, shape, g, a.steps, a.warmup)
               for g in ((12, 13) if a.gen == "both" else (int(a.gen),))}
        if len(res) == 2:
            print(json.dumps({"shape": shape, "tls13_over_tls12_time":
                              {op: round(res[13][op] / res[12][op], 4) for op in ("seal", "open")}}),
                  flush=True)
    engine.close()


if __name__ == "__main__":
    main()
