"""Everything tg::run_batch (talos_amd/csrc/batch.cpp) decides, pinned on the CPU.

The engine's unmodified host objects run against the recording HIP stub
(tests/devstub/devstub.cpp, as in test_device_affinity.py) with its launch
trace on: between devstub_trace_begin and devstub_trace_take every launcher,
allocation call, async memset / copy and stream synchronize appends one line
with its name and all its arguments: every field of BatchArgs, the launcher's
own scalars, sizes in full, pointers as a<k>+<byte offset> into the k-th
allocation first seen in that trace.  So which launchers run, in which order,
with which BatchArgs, which scratch size and which scratch offsets is visible
without a GPU, and a wrong size or offset shows here instead of as an
out-of-bounds device write.

One child process per environment setting (the knobs are read once per
process).  A child drives its cases through the public C ABI, traces only the
call under test (installs and uploads happen outside the trace, each case on a
fresh engine, so the scratch request shows as an allocation size) and prints
12 hex digits of SHA-256 over each case's trace.  The digests are compared with
tests/golden/batch_plan_trace.json, recorded by tests/golden/make_golden.py
--batch-plan from the engine sources of commit 24b4793, BEFORE run_batch was
split into plan_batch + execution (only this stub's trace added); the refactor
had to reproduce every one, and so has every later change that means to keep
the launches.  One change meant not to: under TLSGPU_CHACHA_LEGACY=1 a TLS 1.2
batch of RFC 7905 ChaCha sessions only was planned as fused (no bounds pass, no
initial statuses) although the per-lane kernel that switch selects has neither,
so a record outside the caller's buffers was processed
(test_gpu_tag_len.py::test_legacy_chacha_kernel_forced); plan_batch now keeps
such a batch unfused, and that child's 20 "12:c" digests were recorded again
from the fixed sources.  No other digest moved.

The stub reports 256 CUs: the automatic split threshold is n = 512.
Case ids: b/<generation>:<kinds>/<s|o>/<n>/h<hints>/<impl> for the batch entry
points (kinds: a AES-128, A AES-256, c ChaCha RFC 7905, o ChaCha draft, C the
TLS 1.3 ChaCha kind), w/ wire, h/ host-resident, q/ the EVP coalescing queue.
The stub has no launchers for the experimental kernels (make EXPERIMENTAL=1),
so that #ifdef branch of run_batch is not covered here.
"""
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "devstub")
STUB_LIB = os.path.join(STUB_DIR, "libtlsgpu_devstub.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_plan_trace.json")

# child name -> its environment.  "default" runs the full matrix, the others
# the reduced one (n in {513, 4096}, impl auto and queue, hints 0 and 3, plus
# the child's few extra shapes).
CHILDREN = {
    "default": {},
    "FUSED=0": {"TLSGPU_FUSED": "0"},
    "PACK=0": {"TLSGPU_PACK": "0"},
    "PACK=1": {"TLSGPU_PACK": "1"},
    "PWS=0": {"TLSGPU_PWS": "0"},
    "PWS=1": {"TLSGPU_PWS": "1"},
    "BALANCE=1": {"TLSGPU_BALANCE": "1"},
    "BALANCE=2": {"TLSGPU_BALANCE": "2"},
    "BALANCE=2,SNAP=64": {"TLSGPU_BALANCE": "2", "TLSGPU_BALANCE_SNAP": "64"},
    "PIECES=0": {"TLSGPU_PIECES": "0"},
    "PIECES=2": {"TLSGPU_PIECES": "2"},
    "WG_PER_CU=2": {"TLSGPU_WG_PER_CU": "2"},
    "WG_PER_CU=9": {"TLSGPU_WG_PER_CU": "9"},       # clamps to 4
    "PRE_POOL=1": {"TLSGPU_PRE_POOL": "1"},
    "GCM_IMPL=ttable": {"TLSGPU_GCM_IMPL": "ttable"},
    "GCM_IMPL=hybrid": {"TLSGPU_GCM_IMPL": "hybrid"},  # not built: falls back to auto
    "CHACHA_LEGACY=1": {"TLSGPU_CHACHA_LEGACY": "1"},
    "WG_TIMES=1": {"TLSGPU_WG_TIMES": "1"},
    "BS16_MIN=4096": {"TLSGPU_BS16_MIN": "4096"},
    "HY_FLAGS=2": {"TLSGPU_HY_FLAGS": "2"},
    "BS_RESERVE=1": {"TLSGPU_BS_RESERVE": "1"},
}

_CHILD = r"""
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import talos_amd as ta
FULL = sys.argv[2] == "default"
DUMP = set(sys.argv[3:])          # case ids whose whole trace is printed too
lib = ta.load_library()
lib.devstub_trace_begin.restype = None
lib.devstub_trace_begin.argtypes = [C.c_int]
lib.devstub_trace_take.restype = C.c_size_t
lib.devstub_trace_take.argtypes = [C.c_char_p, C.c_size_t]
_buf = C.create_string_buffer(1 << 20)

def traced(case, fn, all_threads=False):
    lib.devstub_trace_begin(int(all_threads))
    try:
        fn()
    finally:
        n = lib.devstub_trace_take(_buf, len(_buf))
    assert 0 < n < len(_buf), (case, n)
    text = _buf.value.decode()
    print("CASE", case, hashlib.sha256(text.encode()).hexdigest()[:12])
    if case in DUMP:
        print(text, end="")

KIND = {"a": ta.AES_128_GCM, "A": ta.AES_256_GCM, "c": ta.CHACHA20_POLY1305,
        "o": ta.CHACHA20_POLY1305_OLD, "C": ta.CHACHA20_POLY1305_TLS13}
TABLES = [(12, k) for k in ("a", "A", "aA", "c", "o", "co", "ac", "aAco")] + \
         [(13, k) for k in ("a", "C", "aAC")]
IMPL = {"a": "auto", "q": "queue", "t": "ttable", "s": "split"}

def table(eng, gen, kinds):
    tab = ta.SessionTable(eng, 8)
    ps = []
    for k in range(8):
        kind = KIND[kinds[k % len(kinds)]]
        iv = 12 if gen == 13 else ta.FIXED_IV_LEN[kind]
        ps.append(ta.SessionParams(kind, bytes([k + 1]) * ta.KEY_LEN[kind], bytes([k + 7]) * iv,
                                   version=ta.TLS13_VERSION if gen == 13 else 0x0303))
    tab.install(0, ps)
    return tab

def records(n, body):
    r = np.zeros(n, dtype=ta.RECORD_DTYPE)
    i = np.arange(n, dtype=np.uint64)
    r["in_off"] = i * np.uint64(body + 64)
    r["out_off"] = i * np.uint64(body + 64)
    r["seq"] = i
    r["session"] = (i // np.uint64(16)) % np.uint64(8)
    r["len_type"] = (23 << 24) | body
    return r

# device buffers shared by the cases (made outside every trace, on an engine of
# their own): the kernels do not run, so only the descriptors are real
NMAX = 65536
E0 = ta.Engine(0)
IN_BYTES, OUT_BYTES = 1 << 16, 1 << 17
d_recs, d_in, d_out, d_st = (ta.DeviceBuffer(E0, n) for n in (32 * NMAX, IN_BYTES, OUT_BYTES, 4 * NMAX))
d_recs.upload(records(NMAX, 1024).view(np.uint8))

def fresh(gen, kinds, hints):
    eng = ta.Engine(0)
    tab = table(eng, gen, kinds)
    tab.hint(hints)
    return eng, tab

def done(eng, tab):
    tab.close()
    eng.close()

# the process-wide lazy state (TLSGPU_WG_TIMES buffer) before the first case
eng, tab = fresh(12, "a", 0)
ta.seal_batch(tab, d_recs.ptr, 64, d_in.ptr, IN_BYTES, d_out.ptr, OUT_BYTES, d_st.ptr)
done(eng, tab)

# --- tlsgpu_seal_batch / tlsgpu_open_batch
def shapes(impl):
    for seal in (True, False):
        for n in (1, 512, 513, 4096, 65536) if FULL else (513, 4096):
            for hints in (0, 1, 2, 3) if FULL else (0, 3):
                yield seal, n, hints
    if not FULL and impl == "a":
        # what the reduced matrix cannot reach, seal only: hints 2 (SESSION_RUNS
        # alone: fused with the pack variant, where TLSGPU_BALANCE=1 and
        # TLSGPU_PIECES=0 differ from the default) and 65,536 records (more
        # than 16 per workgroup, where TLSGPU_WG_PER_CU changes the grid)
        yield from ((True, n, hints) for n, hints in ((513, 2), (4096, 2), (65536, 2), (65536, 3)))

# (the first impl is never set: it is the one seeded from TLSGPU_GCM_IMPL)
for impl in ("a", "q", "t", "s") if FULL else ("a", "q"):
    if impl != "a":
        ta.set_gcm_impl(IMPL[impl])
    for gen, kinds in TABLES:
        for seal, n, hints in shapes(impl):
            eng, tab = fresh(gen, kinds, hints)
            fn = ta.seal_batch if seal else ta.open_batch
            traced(f"b/{gen}:{kinds}/{'s' if seal else 'o'}/{n}/h{hints}/{impl}",
                   lambda: fn(tab, d_recs.ptr, n, d_in.ptr, IN_BYTES, d_out.ptr, OUT_BYTES,
                              d_st.ptr))
            done(eng, tab)
if not FULL:
    sys.exit(0)
ta.set_gcm_impl("auto")

# --- tlsgpu_open_wire / tlsgpu_seal_wire: the engine's own descriptors (open:
# no bounds, type_out on a TLS 1.3 table), hints from the table
NS = 4
d_wrecs, d_res, d_tot = ta.DeviceBuffer(E0, 32 * 1000), ta.DeviceBuffer(E0, 32 * NS), ta.DeviceBuffer(E0, 4)
ws = np.zeros(NS, dtype=ta.WIRE_STREAM_DTYPE)
wr = np.zeros(NS, dtype=ta.WRITE_STREAM_DTYPE)
for i in range(NS):
    ws[i] = (i * 8192, 4096, i, 0, 0x0303, 0, 0)
    wr[i] = (i * 8192, i * 16384, 0, 4096, i, 0x0303, 23, 0, 0)
d_ws, d_wr = ta.DeviceBuffer(E0, ws.nbytes), ta.DeviceBuffer(E0, wr.nbytes)
d_ws.upload(ws.view(np.uint8))
d_wr.upload(wr.view(np.uint8))
for gen, kinds in ((12, "aAco"), (12, "a"), (12, "c"), (13, "aAC"), (13, "a"), (13, "C")):
    for maxrec in (64, 1000):
        for hints in (0, 3):
            eng, tab = fresh(gen, kinds, hints)
            traced(f"w/{gen}:{kinds}/o/{maxrec}/h{hints}",
                   lambda: ta.open_wire(tab, d_ws.ptr, NS, d_in.ptr, maxrec, d_wrecs.ptr, d_st.ptr,
                                        d_res.ptr, d_tot.ptr))
            done(eng, tab)
            eng, tab = fresh(gen, kinds, hints)
            traced(f"w/{gen}:{kinds}/s/{maxrec}/h{hints}",
                   lambda: ta.seal_wire(tab, d_wr.ptr, NS, d_in.ptr, IN_BYTES, d_out.ptr, OUT_BYTES,
                                        maxrec, d_wrecs.ptr, d_st.ptr, d_res.ptr, d_tot.ptr))
            done(eng, tab)

# --- tlsgpu_open_host / tlsgpu_seal_host: hints from the records (host_hints),
# short (256 B) and long (4 KiB) ones; 3,000 long records make several chunks
def pinned(nbytes):
    p = C.c_void_p()
    assert lib.tlsgpu_host_alloc(E0.handle, nbytes, C.byref(p)) == 0
    return p.value
HB = 3000 * (4096 + 64) + 4096
h_in, h_out, h_st = pinned(HB), pinned(HB), pinned(4 * 3000)
for gen, kinds in ((12, "aAco"), (12, "a"), (12, "c"), (13, "aAC"), (13, "C")):
    for seal in (True, False):
        for n, body in ((64, 256), (700, 256), (700, 4096), (3000, 4096)):
            recs = records(n, body)
            eng, tab = fresh(gen, kinds, 0)
            fn = ta.seal_host if seal else ta.open_host
            traced(f"h/{gen}:{kinds}/{'s' if seal else 'o'}/{n}x{body}",
                   lambda: fn(tab, recs.ctypes.data, n, h_in, HB, h_out, HB, h_st))
            done(eng, tab)

# --- the EVP coalescing queue: raw jobs, launched by the queue's dispatcher
# thread (so every thread is traced), the kinds mask of the jobs in the batch.
# Each context's first call (its deferred install) runs outside the trace.
ta.evp_set_batching(50, 0, 64)
ctxs = {"a": ta.EvpAead(ta.AES_128_GCM, b"k" * 16), "A": ta.EvpAead(ta.AES_256_GCM, b"k" * 32),
        "c": ta.EvpAead(ta.CHACHA20_POLY1305, b"k" * 32),
        "o": ta.EvpAead(ta.CHACHA20_POLY1305_OLD, b"k" * 32)}
for k, ctx in ctxs.items():
    nonce = bytes(8 if k == "o" else 12)
    assert ctx.seal(nonce, b"x" * 64, b"ad")[0] == 1
    traced(f"q/{k}/s", lambda: ctx.seal(nonce, b"x" * 1400, b"ad"), all_threads=True)
    traced(f"q/{k}/o", lambda: ctx.open(nonce, b"y" * 1416, b"ad"), all_threads=True)
"""


def build_stub():
    subprocess.run(["make", "-C", STUB_DIR, "-s"], check=True, capture_output=True)
    return STUB_LIB


def run_child(name, dump=()):
    """{case id: digest} of one child, and its whole output."""
    env = dict(os.environ, TLSGPU_LIBRARY=STUB_LIB, TLSGPU_STUB_DEVICES="1",
               TLSGPU_EVP_DOORBELL="0")
    for k in [k for k in env if k.startswith("TLSGPU_") and
              k not in ("TLSGPU_LIBRARY", "TLSGPU_STUB_DEVICES", "TLSGPU_EVP_DOORBELL")]:
        env.pop(k)
    env.update(CHILDREN[name])
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, *dump], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, name + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
    cases = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            _, cid, digest = line.split()
            assert cid not in cases, cid
            cases[cid] = digest
    return cases, r.stdout


def run_children():
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(CHILDREN, ex.map(lambda n: run_child(n)[0], CHILDREN)))


@pytest.fixture(scope="module")
def stub_lib():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available to build the stub library")
    return build_stub()


def test_run_batch_launches_match_the_recorded_plan(stub_lib):
    golden = json.load(open(GOLDEN))
    assert set(golden) == set(CHILDREN)
    got = run_children()
    bad = []
    for child, want in golden.items():
        # every recorded case ran (a child that stopped early fails here), none is new
        assert set(got[child]) == set(want), (child, sorted(set(want) ^ set(got[child]))[:10])
        bad += [(child, cid) for cid in want if got[child][cid] != want[cid]]
    for child in sorted({c for c, _ in bad}):
        ids = [cid for c, cid in bad if c == child]
        print(f"--- {child}: {len(ids)} cases differ from the recorded plan: "
              f"{' '.join(ids[:12])}{' ...' if len(ids) > 12 else ''}")
        shown, show = ids[:2], False      # the whole trace of the first two
        for line in run_child(child, shown)[1].splitlines():
            if line.startswith("CASE "):
                show = line.split()[1] in shown
            if show:
                print(line)
    assert not bad, f"{len(bad)} cases differ, first: {bad[:8]}"
