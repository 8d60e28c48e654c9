"""tlsgpu_read_wire's host half without a GPU: the engine's host objects over the
recording HIP stub (tests/devstub, as test_gather_wire_host.py).  Every argument
error reaches no HIP call at all: a null argument, d_app overlapping d_wire, a
TLS 1.3 table.  The stub's launcher list has no read launchers (they are weak
references in host_paths.cpp), so a valid call there must fail loudly, again
before any HIP call: a library without the kernels never pretends to have read."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "devstub")
STUB_LIB = os.path.join(STUB_DIR, "libtlsgpu_devstub.so")

_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import talos_amd as ta
lib = ta.load_library()
lib.devstub_trace_begin.restype = None
lib.devstub_trace_begin.argtypes = [C.c_int]
lib.devstub_trace_take.restype = C.c_size_t
lib.devstub_trace_take.argtypes = [C.c_char_p, C.c_size_t]
buf = C.create_string_buffer(1 << 16)
eng = ta.Engine(0)
tab = ta.SessionTable(eng, 1)
tab.install(0, [ta.SessionParams(ta.CHACHA20_POLY1305, bytes(32), bytes(12))])
tab13 = ta.SessionTable(eng, 1)
tab13.install(0, [ta.SessionParams(ta.AES_128_GCM, bytes(16), bytes(12), version=0x0304)])
N, R, WIRE, APP = 3, 100, 65536, 2048
d_streams, d_results, d_recs, d_status, d_wire, d_reads, d_app, d_out, d_total = (
    ta.DeviceBuffer(eng, n) for n in (32 * N, 32 * N, 32 * R, 4 * R, WIRE, 16 * N, APP, 32 * N, 4))

def call(table=tab, n_streams=N, max_records=R, **null):
    a = dict(streams=d_streams.ptr, wire=d_wire.ptr, recs=d_recs.ptr, status=d_status.ptr,
             results=d_results.ptr, total=d_total.ptr, reads=d_reads.ptr, app=d_app.ptr,
             out=d_out.ptr)
    a.update(null)
    lib.devstub_trace_begin(0)
    rc = lib.tlsgpu_read_wire(table.handle if table else None, a["streams"], n_streams, a["wire"],
                              WIRE, max_records, a["recs"], a["status"], a["results"], a["total"],
                              a["reads"], a["app"], APP, a["out"], None)
    lib.devstub_trace_take(buf, len(buf))
    print("RC", rc, lib.tlsgpu_last_error().decode())
    print(buf.value.decode(), end="")
    print("END")

call()                                        # 0: valid, but this library has no read kernels
call(app=d_wire.ptr + WIRE - 1)               # 1: d_app begins on d_wire's last byte
call(app=d_wire.ptr - APP + 1)                # 2: d_app ends on d_wire's first byte
call(table=tab13)                             # 3: a TLS 1.3 table
call(table=None)                              # 4..: a null argument
for name in ("streams", "wire", "recs", "status", "results", "total", "reads", "app", "out"):
    call(**{name: None})
call(n_streams=0, total=None)                 # d_total is needed by the empty call too
call(n_streams=0)                             # the empty call, on a library without the kernels
"""

NULLS = 1 + 9 + 1


@pytest.fixture(scope="module")
def runs():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available to build the stub library")
    subprocess.run(["make", "-C", STUB_DIR, "-s"], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TLSGPU_")}
    env.update(TLSGPU_LIBRARY=STUB_LIB, TLSGPU_STUB_DEVICES="1", TLSGPU_EVP_DOORBELL="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = []
    for block in r.stdout.split("END\n")[:-1]:
        lines = block.splitlines()
        out.append((int(lines[0].split()[1]), lines[1:], lines[0]))
    assert len(out) == 4 + NULLS + 1
    return out


def test_a_library_without_the_kernels_fails_loudly(runs):
    for rc, trace, line in (runs[0], runs[-1]):
        assert rc == -3 and trace == [] and "not linked" in line


@pytest.mark.parametrize("k", [1, 2])
def test_an_overlap_reaches_no_hip_call(runs, k):
    rc, trace, line = runs[k]
    assert rc == -1 and trace == [] and "overlaps" in line


def test_a_tls13_table_reaches_no_hip_call_and_names_the_two_call_path(runs):
    rc, trace, line = runs[3]
    assert rc == -1 and trace == []
    assert "tlsgpu_open_wire" in line and "tlsgpu_gather_wire" in line


@pytest.mark.parametrize("k", range(4, 4 + NULLS))
def test_a_null_argument_reaches_no_hip_call(runs, k):
    rc, trace, line = runs[k]
    assert rc == -1 and trace == [] and "bad arguments" in line
