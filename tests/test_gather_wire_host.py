"""tlsgpu_gather_wire's host half without a GPU: the engine's host objects over
the recording HIP stub (tests/devstub, as test_batch_plan_trace.py).  An
argument error and an empty call reach no HIP call at all.  The stub's launcher
list has no gather launchers (they are weak references in host_paths.cpp), so
a valid call there must fail loudly, again before any HIP call: a library
without the kernels never pretends to have gathered."""
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
N, R, WIRE, APP = 3, 100, 65536, 2048
d_streams, d_results, d_recs, d_status, d_wire, d_reads, d_app, d_out = (
    ta.DeviceBuffer(eng, n) for n in (32 * N, 32 * N, 32 * R, 4 * R, WIRE, 16 * N, APP, 32 * N))

def call(n_streams=N, wire=None, app=None, reads=None, max_records=R):
    lib.devstub_trace_begin(0)
    rc = lib.tlsgpu_gather_wire(tab.handle, d_streams.ptr, d_results.ptr, n_streams, d_recs.ptr,
                                d_status.ptr, max_records, wire or d_wire.ptr, WIRE,
                                d_reads.ptr if reads is None else reads, app or d_app.ptr, APP,
                                d_out.ptr, None)
    lib.devstub_trace_take(buf, len(buf))
    print("RC", rc, lib.tlsgpu_last_error().decode())
    print(buf.value.decode(), end="")
    print("END")

call()                                        # valid, but this library has no gather kernels
call(app=d_wire.ptr + WIRE - 1)               # d_app begins on d_wire's last byte
call(app=d_wire.ptr - APP + 1)                # d_app ends on d_wire's first byte
call(reads=0)                                 # a null argument
call(n_streams=0)                             # the empty call
"""


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
    assert len(out) == 5
    return out


def test_a_library_without_the_kernels_fails_loudly(runs):
    rc, trace, line = runs[0]
    assert rc == -3 and trace == [] and "not linked" in line


@pytest.mark.parametrize("k,why", [(1, "overlaps"), (2, "overlaps"), (3, "bad arguments")])
def test_argument_errors_reach_no_hip_call(runs, k, why):
    rc, trace, line = runs[k]
    assert rc == -1 and trace == [] and why in line


def test_the_empty_call_reaches_no_hip_call(runs):
    rc, trace, _ = runs[4]
    assert rc == 0 and trace == []
