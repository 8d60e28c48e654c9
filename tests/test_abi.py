"""CPU-side checks of the C-ABI library: it loads without a GPU and exports
every function include/*.h declares (no compute calls here)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import talos_amd
    if not os.path.exists(talos_amd.LIBPATH):
        talos_amd.build()
    return talos_amd.load_library()


def test_library_exports_header_symbols(lib):
    import talos_amd
    names = talos_amd.header_symbols()
    assert "tlsgpu_open_batch" in names and "EVP_AEAD_CTX_open" in names
    for n in names:
        assert hasattr(lib, n), n


def test_exports_nothing_else():
    import talos_amd
    out = subprocess.run(["nm", "-D", "--defined-only", talos_amd.LIBPATH], check=True,
                         capture_output=True, text=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert exported == talos_amd.header_symbols()


def test_aead_descriptors_without_gpu(lib):
    """The accessor half of the EVP ABI (evp_aead.c:26-48) needs no device."""
    import talos_amd as ta
    want = {ta.AES_128_GCM: (16, 12, 16, 16), ta.AES_256_GCM: (32, 12, 16, 16),
            ta.CHACHA20_POLY1305: (32, 12, 16, 16), ta.CHACHA20_POLY1305_OLD: (32, 8, 16, 16)}
    for kind, getter in ta.EvpAead.GETTERS.items():
        a = getattr(lib, getter)()
        got = (lib.EVP_AEAD_key_length(a), lib.EVP_AEAD_nonce_length(a),
               lib.EVP_AEAD_max_overhead(a), lib.EVP_AEAD_max_tag_len(a))
        assert got == want[kind]


def test_evp_cipher_objects_without_gpu(lib):
    """EvpCipher's ctypes layouts against the EVP_aes_*_gcm objects (e_aes.c:1049-1059):
    the fields read back, and the ctrls that need no key run on the host alone."""
    import talos_amd as ta
    E = ta.EvpCipher
    for kind, nid, key_len in ((ta.AES_128_GCM, 895, 16), (ta.AES_256_GCM, 901, 32)):
        c = E(kind, False)
        ci = c.cipher
        assert c.ok == 1
        assert (ci.nid, ci.block_size, ci.key_len, ci.iv_len) == (nid, 1, key_len, 12)
        assert ci.flags & 0x7 == 0x6 and ci.flags & 0x200000 and 0 < ci.ctx_size <= 4096
        assert c.ctx.key_len == key_len and c.ctx.encrypt == 0
        assert c.ctrl(E.GCM_SET_IVLEN, 0) == 0 and c.ctrl(E.GCM_SET_IVLEN, 60) == 1
        assert c.ctrl(E.GCM_SET_TAG, 17, bytes(17)) == 0
        assert c.ctrl(E.GCM_SET_TAG, 12, bytes(range(12))) == 1
        assert bytes(c.ctx.buf)[:12] == bytes(range(12))
        assert c.get_tag(16)[0] == 0          # a decrypting context gives no tag
        assert c.update(b"x")[0] == -1        # no key yet
        d = c.copy()                          # nothing on the device to copy yet
        assert d.ok == 1 and d.ctx.cipher_data != c.ctx.cipher_data
        assert d.cleanup() == 1 and c.cleanup() == 1 and c.cleanup() == 1


def test_record_descriptor_layout():
    import talos_amd as ta
    import numpy as np
    assert ta.RECORD_DTYPE.itemsize == 32
    r = np.zeros(1, dtype=ta.RECORD_DTYPE)
    r[0] = (1, 2, 3, 4, ta.len_type(16384, 23))
    raw = r.view(np.uint8)
    assert raw[24] == 4 and int.from_bytes(raw[28:32].tobytes(), "little") == (23 << 24) | 16384


def test_engine_create_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import talos_amd as ta
    with pytest.raises(ta.TlsGpuError):
        ta.Engine(0)


def test_gcm_impl_selection_without_gpu(lib):
    """tlsgpu_set/get_gcm_impl (include/tlsgpu.h): the default build selects
    auto (split for small batches, queue above) and accepts split / queue /
    ttable; the slower experimental kernels are refused unless built."""
    import talos_amd as ta
    prev = ta.get_gcm_impl()
    try:
        for name in ("auto", "split", "queue", "ttable"):
            ta.set_gcm_impl(name)
            assert ta.get_gcm_impl() == name
        assert lib.tlsgpu_set_gcm_impl(99) != 0  # unknown impl: an error code, selection kept
        assert ta.get_gcm_impl() == "ttable"
    finally:
        ta.set_gcm_impl(prev)
    if not os.environ.get("TLSGPU_GCM_IMPL"):
        assert prev == "auto"


def test_sessions_hint_rejects_bad_arguments(lib):
    """tlsgpu_sessions_hint: a null table or an unknown hint bit is EINVAL (no GPU needed)."""
    import ctypes as C
    lib.tlsgpu_sessions_hint.argtypes = [C.c_void_p, C.c_uint]
    lib.tlsgpu_sessions_hint.restype = C.c_int
    assert lib.tlsgpu_sessions_hint(None, 1) != 0
