"""The device key schedule's host side without a GPU (include/tlsgpu.h:
tlsgpu_sessions_install_secrets, tlsgpu_sessions_key_update,
tlsgpu_wire_key_update_ids), over the recording HIP stub (tests/devstub, as
test_wire_key_update_host.py): the new struct's size, null arguments, n == 0,
and every argument error answered BEFORE any HIP call.  The stub's launcher list
has none of the new kernels (weak references in engine.cpp), so a call that
passes its checks answers TLSGPU_EHIP there, also before any HIP call.

A plain tlsgpu_sessions_install makes exactly the HIP calls it made before the
key schedule existed: tests/golden/session_install_trace.json is the stub's
trace of the same calls recorded at the commit before (this file run as a
script against that commit's tree, see the end of the file)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "devstub")
STUB_LIB = os.path.join(STUB_DIR, "libtlsgpu_devstub.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "session_install_trace.json")
EINVAL, EHIP, ERANGE = -1, -3, -4

# the part the commit before can run too: its output is the golden file
_INSTALLS = r"""
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

def traced(name, fn):
    lib.devstub_trace_begin(0)
    rc = fn()
    lib.devstub_trace_take(buf, len(buf))
    print("CALL", name, rc)
    print(buf.value.decode(), end="")
    print("END")

def raw_install(tab, first, params):
    arr = (ta._SessionParams * len(params))(*[p.to_c() for p in params])
    return lib.tlsgpu_sessions_install(tab.handle, first, len(params), arr)

t13 = ta.SessionTable(eng, 8)
t12 = ta.SessionTable(eng, 8)
P13 = [ta.SessionParams(ta.AES_128_GCM, bytes(16), bytes(12), version=0x0304),
       ta.SessionParams(ta.AES_256_GCM, bytes(32), bytes(12), version=0x0304, pad_block=512),
       ta.SessionParams(ta.CHACHA20_POLY1305_TLS13, bytes(32), bytes(12), version=0x0304)]
P12 = [ta.SessionParams(ta.AES_128_GCM, bytes(16), bytes(4)),
       ta.SessionParams(ta.CHACHA20_POLY1305, bytes(32), bytes(12))]
traced("install13", lambda: raw_install(t13, 1, P13))
traced("install13_again", lambda: raw_install(t13, 5, P13[:1]))
traced("install12", lambda: raw_install(t12, 0, P12))
"""

_CHILD = _INSTALLS + r"""
def secrets(tab, first, params, n=None):
    arr = (ta._SecretParams * max(len(params), 1))(*[p.to_c() for p in params])
    return lib.tlsgpu_sessions_install_secrets(tab.handle, first, len(params) if n is None else n, arr)

S = ta.SecretParams
ok128, ok256, okcc = S(ta.AES_128_GCM, bytes(32)), S(ta.AES_256_GCM, bytes(48)), \
    S(ta.CHACHA20_POLY1305_TLS13, bytes(32), pad_block=512)
print("SIZEOF", C.sizeof(ta._SecretParams))
fresh = ta.SessionTable(eng, 8)
ids, st = ta.DeviceBuffer(eng, 64), ta.DeviceBuffer(eng, 64)
traced("null_table", lambda: lib.tlsgpu_sessions_install_secrets(None, 0, 0, None))
traced("null_params", lambda: lib.tlsgpu_sessions_install_secrets(fresh.handle, 0, 1, None))
traced("n0", lambda: secrets(fresh, 0, [], 0))
traced("n0_null", lambda: lib.tlsgpu_sessions_install_secrets(fresh.handle, 8, 0, None))
traced("len_mismatch_128", lambda: secrets(fresh, 0, [ok256, S(ta.AES_128_GCM, bytes(48))]))
traced("len_mismatch_256", lambda: secrets(fresh, 0, [S(ta.AES_256_GCM, bytes(32))]))
traced("len_mismatch_cc", lambda: secrets(fresh, 0, [S(ta.CHACHA20_POLY1305_TLS13, bytes(48))]))
traced("len_zero", lambda: secrets(fresh, 0, [S(ta.AES_128_GCM, b"")]))
traced("kind_tls12_chacha", lambda: secrets(fresh, 0, [S(ta.CHACHA20_POLY1305, bytes(32))]))
traced("kind_tls12_chacha_old", lambda: secrets(fresh, 0, [S(ta.CHACHA20_POLY1305_OLD, bytes(32))]))
traced("kind_unknown", lambda: secrets(fresh, 0, [S(0, bytes(32))]))
traced("pad_block_3", lambda: secrets(fresh, 0, [S(ta.AES_128_GCM, bytes(32), pad_block=3)]))
traced("pad_block_32768", lambda: secrets(fresh, 0, [S(ta.AES_128_GCM, bytes(32), pad_block=32768)]))
traced("range", lambda: secrets(fresh, 6, [ok128, ok256, okcc]))
traced("range_first", lambda: secrets(fresh, 0xFFFFFFFF, [ok128, ok256]))
traced("tls12_table", lambda: secrets(t12, 4, [ok128]))
traced("valid_without_kernels", lambda: secrets(fresh, 0, [ok128, ok256, okcc]))
# ... which left the table as it was: it still takes either generation
traced("fresh_still_fresh", lambda: raw_install(fresh, 0, P12))

ku = lib.tlsgpu_sessions_key_update
traced("ku_null_table", lambda: ku(None, ids.ptr, 1, st.ptr, None))
traced("ku_null_ids", lambda: ku(t13.handle, None, 1, st.ptr, None))
traced("ku_null_status", lambda: ku(t13.handle, ids.ptr, 1, None, None))
traced("ku_n0", lambda: ku(t13.handle, None, 0, None, None))
traced("ku_without_kernels", lambda: ku(t13.handle, ids.ptr, 4, st.ptr, None))
wi = lib.tlsgpu_wire_key_update_ids
traced("ids_null_table", lambda: wi(None, ids.ptr, ids.ptr, 1, ids.ptr, None))
traced("ids_null_streams", lambda: wi(t13.handle, None, ids.ptr, 1, ids.ptr, None))
traced("ids_null_results", lambda: wi(t13.handle, ids.ptr, None, 1, ids.ptr, None))
traced("ids_null_ids", lambda: wi(t13.handle, ids.ptr, ids.ptr, 1, None, None))
traced("ids_n0", lambda: wi(t13.handle, None, None, 0, None, None))
traced("ids_without_kernels", lambda: wi(t13.handle, ids.ptr, ids.ptr, 1, ids.ptr, None))
# tables that hold no key-schedule scratch are destroyed with the calls they always made
traced("destroy", lambda: (t13.close(), 0)[1])
"""


def parse(stdout):
    """{name: (rc, [trace lines])} and the lines outside the blocks"""
    calls, loose, cur = {}, [], None
    for line in stdout.splitlines():
        if line.startswith("CALL "):
            _, name, rc = line.split()
            cur = calls[name] = (int(rc), [])
        elif line == "END":
            cur = None
        elif cur is not None:
            cur[1].append(line)
        else:
            loose.append(line)
    return calls, loose


def run_child(code, root=ROOT, stub=STUB_LIB):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TLSGPU_")}
    env.update(TLSGPU_LIBRARY=stub, TLSGPU_STUB_DEVICES="1", TLSGPU_EVP_DOORBELL="0")
    r = subprocess.run([sys.executable, "-c", code, root], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return parse(r.stdout)


@pytest.fixture(scope="module")
def runs():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available to build the stub library")
    subprocess.run(["make", "-C", STUB_DIR, "-s"], check=True, capture_output=True)
    return run_child(_CHILD)


def test_secret_params_is_60_bytes(runs):
    import talos_amd as ta
    assert C.sizeof(ta._SecretParams) == 60
    assert runs[1] == ["SIZEOF 60"]
    assert (ta._SecretParams.secret.offset, ta._SecretParams.pad_block.offset) == (8, 56)
    assert (ta.SESSION_NONE, ta.REKEY_SKIPPED) == (0xFFFFFFFF, 1)


def test_null_arguments_are_einval_and_n0_is_ok(runs):
    calls = runs[0]
    for name in ("null_table", "null_params", "ku_null_table", "ku_null_ids", "ku_null_status",
                 "ids_null_table", "ids_null_streams", "ids_null_results", "ids_null_ids"):
        assert calls[name] == (EINVAL, []), name
    for name in ("n0", "n0_null", "ku_n0", "ids_n0"):
        assert calls[name] == (0, []), name


@pytest.mark.parametrize("name,rc", [
    ("len_mismatch_128", EINVAL), ("len_mismatch_256", EINVAL), ("len_mismatch_cc", EINVAL),
    ("len_zero", EINVAL), ("kind_tls12_chacha", EINVAL), ("kind_tls12_chacha_old", EINVAL),
    ("kind_unknown", EINVAL), ("pad_block_3", EINVAL), ("pad_block_32768", EINVAL),
    ("range", ERANGE), ("range_first", ERANGE), ("tls12_table", EINVAL)])
def test_rejected_before_any_hip_call(runs, name, rc):
    assert runs[0][name] == (rc, [])


def test_a_library_without_the_kernels_says_so_before_any_hip_call(runs):
    calls = runs[0]
    for name in ("valid_without_kernels", "ku_without_kernels", "ids_without_kernels"):
        assert calls[name] == (EHIP, []), name
    # the refused install did not fix the table's generation
    assert calls["fresh_still_fresh"][0] == 0


def test_plain_install_makes_the_hip_calls_it_always_made(runs):
    golden = json.load(open(GOLDEN))
    for name in ("install13", "install13_again", "install12"):
        rc, trace = runs[0][name]
        assert rc == 0 and trace == golden[name], name
        names = [l.split()[0] for l in trace]
        assert names == ["hipMalloc", "hipMemcpyAsync", "launch_session_install", "hipMemsetAsync",
                         "hipStreamSynchronize", "hipFree"]
    rc, trace = runs[0]["destroy"]
    assert [l.split()[0] for l in trace] == golden["destroy_calls"]


if __name__ == "__main__":
    # record the golden file: run at the commit BEFORE the key schedule, with
    # that commit's tree as argv[1] (its stub library built)
    root = sys.argv[1]
    code = _INSTALLS + 'traced("destroy", lambda: (t13.close(), 0)[1])\n'
    calls, _ = run_child(code, root, os.path.join(root, "tests", "devstub", "libtlsgpu_devstub.so"))
    out = {k: v[1] for k, v in calls.items() if k != "destroy"}
    out["destroy_calls"] = [l.split()[0] for l in calls["destroy"][1]]
    json.dump(out, open(GOLDEN, "w"), indent=1)
    print(json.dumps(out, indent=1))
