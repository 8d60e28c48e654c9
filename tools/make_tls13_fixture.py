#!/usr/bin/env python3
"""Capture TLS 1.3 records from a real connection: tests/golden/tls13_wire.json.

Python's ssl module (the system OpenSSL) runs a TLS 1.3 handshake between a
client and a server over two MemoryBIOs with tests/golden/server.pem, then
each side writes application data of several lengths, among them one write of
more than 16 KiB (several records).  The key log gives CLIENT_TRAFFIC_SECRET_0
and SERVER_TRAFFIC_SECRET_0; HKDF-Expand-Label (tests/tls13_helper.py) gives
each direction's write key and IV.  Every protected record of either
direction that opens under those keys at the running sequence number is
written out: suite, key, IV, the lengths of the writes and per record seq, wire
bytes (header + fragment), inner content type and content (byte strings in
base64).  The server's NewSessionTicket
records (inner type 22) are part of its direction; records under the
handshake keys do not open and are left out.

The AEAD used to open the records here is the oracle's; the test suite then
checks the helper's seal against the captured bytes, and the engine against
both.  usage: tools/make_tls13_fixture.py [--suite SUITE] [out.json]

--suite TLS_CHACHA20_POLY1305_SHA256 writes tests/golden/tls13_wire_chacha.json
in the same format with the same writes.  Python's ssl cannot choose TLS 1.3
suites, so the tool writes a temporary OpenSSL configuration (system_default ->
Ciphersuites = SUITE) and starts itself as a fresh child process with
OPENSSL_CONF pointing at it; still two MemoryBIOs, no socket.  The records are
opened with the oracle's RFC 7905 AEAD (kind 3: the TLS 1.3 suite's cipher and
nonce are the same), key and IV from HKDF-Expand-Label with SHA-256.

--record-padding N captures the same connection under OpenSSL's block padding
(the RecordPadding configuration command, SSL_CTX_set_block_padding): the
temporary configuration gets a `RecordPadding = N` line, by the same child-process
route, and the output is tests/golden/tls13_wire_padded.json (with --suite
TLS_CHACHA20_POLY1305_SHA256: tls13_wire_chacha_padded.json), the format above
plus "record_padding": N.  Each record's content and inner type are what is
left of the inner plaintext without its zero padding.
"""
import argparse
import base64
import json
import os
import ssl
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import pyoracle as po  # noqa: E402
import tls13_helper as t13  # noqa: E402

PEM = os.path.join(ROOT, "tests", "golden", "server.pem")
GOLDEN_CHACHA = os.path.join(ROOT, "tests", "golden", "tls13_wire_chacha.json")
GOLDEN_PADDED = os.path.join(ROOT, "tests", "golden", "tls13_wire_padded.json")
GOLDEN_CHACHA_PADDED = os.path.join(ROOT, "tests", "golden", "tls13_wire_chacha_padded.json")
# suite -> (oracle AEAD kind, hash of the key schedule); the helper's table and ChaCha
SUITES = dict(t13.SUITES, TLS_CHACHA20_POLY1305_SHA256=(po.CHACHA20_POLY1305, "sha256"))
CHILD_ENV = "MAKE_TLS13_FIXTURE_CHILD"   # set in the child that runs under the suite's config
CLIENT_WRITES = [1, 16, 1008]        # small: the fixture is committed
SERVER_WRITES = [49, 992, 16385]     # the last one goes out as two records


def pattern(n: int, salt: int) -> bytes:
    return bytes((7 * i + 13 * salt + (i >> 8)) & 0xFF for i in range(n))


def traffic_keys(secret: bytes, suite: str):
    kind, hashname = SUITES[suite]
    return (kind, t13.hkdf_expand_label(secret, "key", po.KEY_LEN[kind], hashname),
            t13.hkdf_expand_label(secret, "iv", 12, hashname))


def run_with_suite(suite: str, out_path: str, padding: int = 0) -> None:
    """This tool again, in a fresh process whose OpenSSL offers `suite` alone
    (None: its own choice) and pads records to blocks of `padding` bytes (0: no
    such line)."""
    conf = tempfile.NamedTemporaryFile("w", suffix=".cnf", delete=False)
    conf.write("openssl_conf = openssl_init\n[openssl_init]\nssl_conf = ssl_sect\n"
               "[ssl_sect]\nsystem_default = system_default_sect\n"
               "[system_default_sect]\n")
    if suite:
        conf.write("Ciphersuites = %s\n" % suite)
    if padding:
        conf.write("RecordPadding = %d\n" % padding)
    conf.close()
    try:
        env = dict(os.environ, OPENSSL_CONF=conf.name, **{CHILD_ENV: "1"})
        args = (["--suite", suite] if suite else []) + \
               (["--record-padding", str(padding)] if padding else [])
        subprocess.run([sys.executable, os.path.abspath(__file__), *args, out_path],
                       check=True, env=env)
    finally:
        os.unlink(conf.name)


def main(out_path: str, want_suite: str = None, padding: int = 0) -> None:
    keylog = tempfile.NamedTemporaryFile(suffix=".keylog", delete=False)
    keylog.close()
    sctx = ssl.SSLContext(ssl.PROTOCOL_TLS_SERVER)
    sctx.set_ciphers("ALL:@SECLEVEL=0")   # the test certificate is old
    sctx.load_cert_chain(PEM)
    sctx.minimum_version = ssl.TLSVersion.TLSv1_3
    cctx = ssl.SSLContext(ssl.PROTOCOL_TLS_CLIENT)
    cctx.set_ciphers("ALL:@SECLEVEL=0")
    cctx.check_hostname = False
    cctx.verify_mode = ssl.CERT_NONE
    cctx.minimum_version = ssl.TLSVersion.TLSv1_3
    cctx.keylog_filename = keylog.name
    c_in, c_out, s_in, s_out = (ssl.MemoryBIO() for _ in range(4))
    cli = cctx.wrap_bio(c_in, c_out, server_side=False)
    srv = sctx.wrap_bio(s_in, s_out, server_side=True)
    wire = {"client": b"", "server": b""}

    def pump():
        moved = False
        for name, src, dst in (("client", c_out, s_in), ("server", s_out, c_in)):
            data = src.read()
            if data:
                wire[name] += data
                dst.write(data)
                moved = True
        return moved

    done = [False, False]
    for _ in range(20):
        for k, side in enumerate((cli, srv)):
            if not done[k]:
                try:
                    side.do_handshake()
                    done[k] = True
                except ssl.SSLWantReadError:
                    pass
        pump()
        if all(done):
            break
    assert all(done) and cli.version() == "TLSv1.3", cli.version()
    suite = cli.cipher()[0]
    assert want_suite in (None, suite), (want_suite, suite)
    writes = {"client": [], "server": []}
    for name, side, peer, lens in (("client", cli, srv, CLIENT_WRITES),
                                   ("server", srv, cli, SERVER_WRITES)):
        for k, n in enumerate(lens):
            data = pattern(n, k + (100 if name == "server" else 0))
            side.write(data)
            pump()
            got = b""
            while len(got) < n:
                try:
                    got += peer.read(n - len(got))
                except ssl.SSLWantReadError:
                    break
            assert got == data
            writes[name].append(n)   # the records' contents concatenate to the writes
    secrets = {}
    for line in open(keylog.name):
        f = line.split()
        if len(f) == 3:
            secrets[f[0]] = bytes.fromhex(f[2])
    os.unlink(keylog.name)
    orc = po.Oracle()
    fixture = {"suite": suite, "openssl": ssl.OPENSSL_VERSION, "directions": []}
    if padding:
        fixture["record_padding"] = padding
    for name, label in (("client", "CLIENT_TRAFFIC_SECRET_0"), ("server", "SERVER_TRAFFIC_SECRET_0")):
        kind, key, iv = traffic_keys(secrets[label], suite)
        ctx = orc.aead(kind, key)
        seq, recs = 0, []
        for hdr, frag in t13.split_records(wire[name]):
            if hdr[0] != t13.APPLICATION_DATA:
                continue   # ClientHello / ServerHello / compatibility ChangeCipherSpec
            st, inner = t13.open_fragment(orc, ctx, iv, seq, frag)
            if st < 0:
                assert not recs, "a record after the first application-key record did not open"
                continue   # under the handshake traffic keys
            recs.append({"seq": seq, "wire": base64.b64encode(hdr + frag).decode(),
                         "inner_type": inner[st],
                         "content": base64.b64encode(inner[:st]).decode()})
            seq += 1
        assert recs
        fixture["directions"].append({"name": name, "key": key.hex(), "iv": iv.hex(),
                                      "records": recs, "writes": writes[name]})
    with open(out_path, "w") as f:   # one record per line
        recs = [d.pop("records") for d in fixture["directions"]]
        head = json.dumps(fixture)
        for d, r in zip(fixture["directions"], recs):
            d["records"] = r
            one = json.dumps({k: v for k, v in d.items() if k != "records"})
            head = head.replace(one, one[:-1] + ', "records": [\n' +
                                ",\n".join(json.dumps(x) for x in r) + "]}")
        f.write(head + "\n")
    print(out_path, suite, {d["name"]: len(d["records"]) for d in fixture["directions"]})


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--suite", choices=sorted(SUITES),
                    help="negotiate this TLS 1.3 suite (default: OpenSSL's own choice)")
    ap.add_argument("--record-padding", type=int, default=0, metavar="N",
                    help="capture under OpenSSL's RecordPadding = N (block padding)")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    pad = args.record_padding
    if args.suite is None and not pad:
        main(args.out or t13.GOLDEN)
    else:
        chacha = args.suite is not None and "CHACHA" in args.suite
        out = args.out or ((GOLDEN_CHACHA_PADDED if chacha else GOLDEN_PADDED) if pad
                           else (GOLDEN_CHACHA if chacha else t13.GOLDEN))
        if os.environ.get(CHILD_ENV):
            main(out, args.suite, pad)
        else:
            run_with_suite(args.suite, out, pad)
