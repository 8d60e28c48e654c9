"""Per-call host time of tlsgpu_seal_batch under the recording HIP stub (tests/devstub; kernels do
nothing): usage  python scripts/batch_dispatch_cost.py TREE  (a built checkout with its stub library);
prints ns per call for an {AES-128} table with hints 3 and an all-kinds table with hints 0
(profiles/r11_batch_plan_dispatch.txt)."""
import os, sys, time
import numpy as np
root = sys.argv[1]
os.environ["TLSGPU_LIBRARY"] = os.path.join(root, "tests/devstub/libtlsgpu_devstub.so")
os.environ["TLSGPU_STUB_DEVICES"] = "1"
sys.path.insert(0, root)
import talos_amd as ta
CALLS = 200000
def case(kinds, hints):
    eng = ta.Engine(0)
    tab = ta.SessionTable(eng, 8)
    ps = []
    for k in range(8):
        kind = kinds[k % len(kinds)]
        ps.append(ta.SessionParams(kind, bytes([k + 1]) * ta.KEY_LEN[kind], bytes([7]) * ta.FIXED_IV_LEN[kind]))
    tab.install(0, ps)
    tab.hint(hints)
    n = 64
    r = np.zeros(n, dtype=ta.RECORD_DTYPE)
    for i in range(n):
        r[i] = (i * 2048, i * 2048, i, i % 8, (23 << 24) | 1024)
    BUF = n * 2048
    d_recs, d_in, d_out, d_st = (ta.DeviceBuffer(eng, b) for b in (32 * n, BUF, BUF, 4 * n))
    d_recs.upload(r.view(np.uint8))
    f = tab.lib.tlsgpu_seal_batch
    args = (tab.handle, d_recs.ptr, n, d_in.ptr, BUF, d_out.ptr, BUF, d_st.ptr, None)
    for _ in range(2000):
        f(*args)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        f(*args)
    return (time.perf_counter() - t0) / CALLS * 1e9
a = case([ta.AES_128_GCM], 3)
b = case([ta.AES_128_GCM, ta.AES_256_GCM, ta.CHACHA20_POLY1305, ta.CHACHA20_POLY1305_OLD], 0)
print(f"{a:.1f} {b:.1f}")
