"""Every phase-timing slot of the queue kernel on a bench config (diagnostic).

Runs config B's (or another config's) open batch with TLSGPU_PHASE_STATS=1 and
prints all 16 slots of talos_amd.debug_phase_stats — wave-cycles and events
per launch and cycles per event — including the hand-over slots bench.py's
name table does not know: claim -> descriptor, descriptor -> constants,
constants -> first loads issued (gcm_device.h kLapDesc / kLapConsts /
kLapFirst).  Slots are summed over waves: a share is a slot's cycles over the
sum of the slots that tile a wave's time (barrier, tables, plan, hand-over,
x4 + rest, finish); kLapFirst lies inside tt-x4 and is not added again.
usage: python tools/phase_stats.py [--config B] [--launches 10] [--sessions N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = {0: "claim->desc", 1: "bs-aes", 2: "bs-consume", 3: "bs-finish", 4: "bs-barrier",
         5: "tables", 6: "tt-switch", 7: "desc->consts", 8: "consts->first",
         9: "tt-x4", 10: "tt-rest", 11: "tt-finish", 12: "tt-barrier", 13: "pack",
         14: "recs/pack", 15: "plan"}
INSIDE = {8, 14}   # slot 8 is part of slot 9's interval, slot 14 counts records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--sessions", type=int, default=0, help="override the config's sessions")
    args = ap.parse_args()
    os.environ.setdefault("TLSGPU_PHASE_STATS", "1")
    import bench
    import talos_amd as ta
    from talos_amd.workload import Workload, zipf_lengths
    kind_name, per_gpu, sessions, rec_len, seed, op = bench.CONFIGS[args.config]
    if args.sessions:
        sessions = min(args.sessions, per_gpu)
    ta.load_library()
    eng = ta.Engine(0)
    kind = ta.AEAD_NAMES[kind_name]
    lengths = None if rec_len else zipf_lengths(per_gpu, seed)
    wl = Workload(eng, kind, per_gpu, sessions, seed, lengths=lengths, record_len=rec_len or 0,
                  tamper_every=1024)
    desc_len = wl.lengths + ta.EXPLICIT_NONCE_LEN[kind] + ta.TAG_LEN
    wl.table.hint(ta.batch_hints(desc_len, wl.session, seal=False))
    for _ in range(5):                    # warm-up: clocks and caches as in bench.py
        wl.open(None)
    eng.sync()
    ta.debug_phase_stats(eng, reset=True)
    for _ in range(args.launches):
        wl.open(None)
    eng.sync()
    st = ta.debug_phase_stats(eng, reset=True)
    total = sum(st[2 * i] for i in range(16) if i not in INSIDE)
    print(json.dumps({"config": args.config, "records": per_gpu, "sessions": sessions,
                      "launches": args.launches, "library": ta.LIBPATH}))
    for i in range(16):
        cyc, ev = st[2 * i], st[2 * i + 1]
        if not ev:
            continue
        share = "" if i in INSIDE else f" share {cyc / total:6.3f}"
        print(f"slot {i:2d} {NAMES[i]:14s} cycles/launch {cyc / args.launches:14.0f} "
              f"events/launch {ev / args.launches:9.0f} cycles/event {cyc / ev:9.0f}{share}")
    eng.close()


if __name__ == "__main__":
    main()
