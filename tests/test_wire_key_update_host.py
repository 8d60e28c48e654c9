"""tlsgpu_open_wire's KeyUpdate switch without a GPU: the engine's host objects
over the recording HIP stub (tests/devstub, as test_gather_wire_host.py).  The
switch exists and a null table is TLSGPU_EINVAL; with the switch off — never
touched, or turned on and off again — tlsgpu_open_wire makes exactly the HIP
calls it always made; with it on, a library without the two new kernels (the
stub's launcher list has none: they are weak references in host_paths.cpp)
answers TLSGPU_EHIP before any HIP call, and never pretends to have looked."""
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
N, R, WIRE = 3, 100, 65536
d_streams, d_results, d_recs, d_status, d_wire, d_total = (
    ta.DeviceBuffer(eng, n) for n in (32 * N, 32 * N, 32 * R, 4 * R, WIRE, 4))

def table(params):
    t = ta.SessionTable(eng, 1)
    t.install(0, [params])
    return t

def call(tab, max_records=R, n_streams=N):
    lib.devstub_trace_begin(0)
    rc = lib.tlsgpu_open_wire(tab.handle, d_streams.ptr, n_streams, d_wire.ptr, max_records,
                              d_recs.ptr, d_status.ptr, d_results.ptr, d_total.ptr, None)
    lib.devstub_trace_take(buf, len(buf))
    print("RC", rc, lib.tlsgpu_last_error().decode() if rc else "")
    print(buf.value.decode(), end="")
    print("END")

t13 = table(ta.SessionParams(ta.AES_128_GCM, bytes(16), bytes(12), version=0x0304))
t12 = table(ta.SessionParams(ta.CHACHA20_POLY1305, bytes(32), bytes(12)))
print("SWITCH", lib.tlsgpu_sessions_wire_key_update(None, 1),
      lib.tlsgpu_sessions_wire_key_update(t13.handle, 0))
call(t13)                                            # 0: warms the stream's scratch
call(t13)                                            # 1: the switch never touched
ta.sessions_wire_key_update(t13, True)
call(t13)                                            # 2: on, no kernels in this library
call(t13, max_records=0)                             # 3: on, nothing to cut: still loud
ta.sessions_wire_key_update(t13, False)
call(t13)                                            # 4: off again
call(t12)                                            # 5: warm-up of the TLS 1.2 table's kind
call(t12)                                            # 6: TLS 1.2, never touched
ta.sessions_wire_key_update(t12, True)
call(t12)                                            # 7: TLS 1.2, on: accepted by the switch ...
ta.sessions_wire_key_update(t12, False)
call(t12)                                            # 8: ... and off again
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
    head, _, rest = r.stdout.partition("\n")
    out = [head]
    for block in rest.split("END\n")[:-1]:
        lines = block.splitlines()
        out.append((int(lines[0].split()[1]), lines[1:], lines[0]))
    assert len(out) == 10
    return out


def test_the_switch_exists_and_null_is_einval(runs):
    assert runs[0].split() == ["SWITCH", "-1", "0"]


def test_switch_off_makes_the_same_hip_calls_as_before(runs):
    (rc1, never, _), (rc4, off_again, _) = runs[2], runs[5]
    assert rc1 == 0 and rc4 == 0
    assert never == off_again
    names = [l.split()[0] for l in never]
    # the call's sequence: d_total and the descriptors preset, framing, the open, the finish
    assert names[:3] == ["hipMemsetAsync", "hipMemsetAsync", "launch_wire_frame"]
    assert names[-1] == "launch_wire_finish" and names.count("launch_wire_finish") == 1
    assert not any("peek" in n or "ku_confirm" in n for n in names)


def test_switch_on_without_the_kernels_is_ehip_before_any_hip_call(runs):
    for k in (3, 4):
        rc, trace, line = runs[k]
        assert rc == -3 and trace == [] and "not linked" in line


def test_tls12_table_accepts_the_switch(runs):
    """The switch is per table and no property of the sessions: a TLS 1.2 table
    takes it; off again, its calls are the ones it always made."""
    (rc6, never, _), (rc8, off_again, _) = runs[7], runs[9]
    assert rc6 == 0 and rc8 == 0 and never == off_again
    assert runs[8][0] == -3        # on: this library has no kernels, whatever the table holds
