"""The host logic of the protocol symbols (constantine_amd/csrc/protocols_host.h) on the CPU, without the library and without a GPU:
tests/protocols_harness.cpp is that header behind a command line, and every answer is compared for equality with Python -- hashlib,
the spec restatement oracle/kzg_spec.py, plain integers (oracle/pyoracle.py for Fp2) and tests/_peerdasref.py.  The wire formats
decide about untrusted bytes: the ZCash G1 codec, blob parsing, the c-kzg text reader of the trusted setup (every rejection of
test_kzg_context_from_the_ceremony_text_file and four more) and the EIP-2537 input parser; the body of the cell-quotient kernel runs
lane by lane."""
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from constantine_amd.evm import CttEVMStatus
from constantine_amd.kzg import cttEthKzgStatus, cttEthTrustedSetupStatus
from oracle import kzg_spec as ks
from oracle import pyoracle as po
from tests import _golden

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")
BLOB = ks.BYTES_PER_BLOB
EVM_DOC = json.load(open(os.path.join(_golden.HERE, "eip2537_multiexp.json")))
G2 = po.BLS12_381_G2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_path_factory.mktemp("protocols")), "protocols_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "protocols_harness.cpp"), "-o", exe], check=True)

    def run(*args, data=b"", rc=0):
        p = subprocess.run([exe, *args], input=data, capture_output=True)
        assert p.returncode == rc, (args, p.returncode, p.stderr)
        return p.stdout
    return run


@pytest.fixture(scope="module")
def srs_raw():
    return open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read()


def _le(rows):
    return [int.from_bytes(bytes(r), "little") for r in rows]


def test_eip4844_host_logic(harness, srs_raw):
    """what test_host_logic_of_the_c_symbols asserts of the exported symbols, of the header itself"""
    rng = random.Random(5)
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 1000, 131072 + 64):
        d = bytes(rng.randrange(256) for _ in range(n)) if n < 2000 else os.urandom(n)
        assert harness("sha256", data=d) == hashlib.sha256(d).digest(), n
    ok = bytes([cttEthKzgStatus.cttEthKzg_Success.value])
    for i in list(range(0, 4096, 97)) + [4095]:
        c = srs_raw[48 * i:48 * i + 48]
        aff = ks.aff_mont_bytes(_golden.g1_decompress(c))
        assert harness("decompress", data=c) == ok + aff, i
        assert harness("compress", data=aff) == c, i
    inf = bytes([0xC0]) + bytes(47)
    assert harness("decompress", data=inf) == ok + bytes(96) and harness("compress", data=bytes(96)) == inf
    for bad, want in ((bytes(48), "cttEthKzg_EccInvalidEncoding"),                                    # compression flag missing
                      (bytes([0xE0]) + bytes(47), "cttEthKzg_EccInvalidEncoding"),                   # infinity with the sign bit
                      (bytes([0xC0]) + bytes(46) + b"\x01", "cttEthKzg_EccInvalidEncoding"),         # infinity with payload
                      (bytes([0x9F]) + bytes([0xFF]) * 47, "cttEthKzg_EccCoordinateGreaterThanOrEqualModulus"),
                      (bytes([0x80]) + bytes(46) + b"\x02", "cttEthKzg_EccPointNotOnCurve")):         # x = 2: 12 is not a square
        out = harness("decompress", data=bad)
        assert len(out) == 1 and cttEthKzgStatus(out[0]).name == want, bad.hex()
        with pytest.raises(ks.SpecError) as e:
            ks.deserialize_g1_compressed(bad)
        assert e.value.status == want
    n_bad = 0
    for name, blob, com in _golden.kzg4844_raw_cases():
        if com is None:
            n_bad += 1
            if len(blob) != BLOB:     # (cttEthKzg_InputsLengthsMismatch is the binding's: the C symbol takes a pointer to a whole blob)
                harness("blob", data=blob, rc=2)
            else:
                assert harness("blob", data=blob) == bytes([cttEthKzgStatus.cttEthKzg_ScalarLargerThanCurveOrder.value]), name
        else:
            assert harness("blob", data=blob) == ok + bytes(ks.blob_to_bigint_polynomial(blob)), name
    assert n_bad == 4
    cases = _golden.kzg4844_proof_cases()
    n_challenges = 0
    for case, blob, com, res in cases["compute_blob_kzg_proof"]:
        if len(blob) == BLOB and len(com) == 48:
            assert int.from_bytes(harness("challenge", data=blob + com), "big") == ks.compute_challenge(blob, com), case
            n_challenges += 1
    assert n_challenges >= 5
    checked = roots = 0
    for case, blob, zb, res in cases["compute_kzg_proof"]:
        if res is None:
            continue
        z = int.from_bytes(zb, "big")
        is_root = z in ks.domain_brp()
        if not is_root and checked >= 6:
            continue
        poly = _le(ks.blob_to_bigint_polynomial(blob))
        out = harness("quotient", data=b"".join(v.to_bytes(32, "little") for v in poly) + z.to_bytes(32, "little"))
        assert len(out) == BLOB + 32
        want_q, want_y = ks.quotient_polynomial(poly, z)
        assert int.from_bytes(out[BLOB:], "little") == want_y and want_y.to_bytes(32, "big") == res[1], case
        assert _le(out[32 * i:32 * i + 32] for i in range(4096)) == want_q, case
        checked += 1
        roots += is_root
    assert checked >= 7 and roots >= 1


def test_trusted_setup_text_reader(harness, srs_raw, tmp_path):
    """srs_read_ckzg4844 on the files of test_kzg_context_from_the_ceremony_text_file, which needs a GPU context to reach the same
    reader, and on four more malformed ones"""
    status = {s: bytes([s.value]) for s in cttEthTrustedSetupStatus}
    invalid = status[cttEthTrustedSetupStatus.cttEthTS_InvalidFile]
    # the golden fixture holds the Lagrange section only: the neutral element stands in for the 65 G2 points, the Lagrange lines for
    # the 4096 monomial ones
    g2 = bytes([0xC0]) + bytes(95)
    g2_first = bytes([0x80]) + bytes(46) + b"\x01"      # a first coordinate in range, the compression flag on it
    g1_lines = [srs_raw[48 * i:48 * i + 48].hex() for i in range(4096)]
    head = "4096\n65\n"

    def compose(lagrange=g1_lines, g2_lines=[g2.hex()] * 65, monomial=g1_lines, head=head):
        return head + "".join(ln + "\n" for sec in (lagrange, g2_lines, monomial) for ln in sec)

    def replaced(lines, i, ln):
        return lines[:i] + [ln] + lines[i + 1:]
    text = compose()
    path = tmp_path / "setup.txt"
    path.write_text(text)
    assert harness("srs", str(path)) == status[cttEthTrustedSetupStatus.cttEthTS_Success] + srs_raw
    crlf = tmp_path / "crlf.txt"
    crlf.write_bytes(text.replace("\n", "\r\n").encode())
    assert harness("srs", str(crlf)) == status[cttEthTrustedSetupStatus.cttEthTS_Success] + srs_raw
    assert harness("srs", str(tmp_path / "nope.txt")) == status[cttEthTrustedSetupStatus.cttEthTS_MissingOrInaccessibleFile]
    cases = {
        # the eight of the GPU test
        "non-hex": text.replace(g1_lines[7], "+f" + g1_lines[7][2:], 1),
        "short line": text.replace(g1_lines[9], g1_lines[9][:-2], 1),
        "long line": text.replace(g1_lines[9], g1_lines[9] + "00", 1),
        "no monomial section": compose(monomial=[]),
        "truncated G2 section": compose(g2_lines=[g2.hex()] * 10, monomial=[]),
        "G2 without the compression flag": text.replace(g2.hex(), "00" * 96, 1),
        "wrong count": text.replace("4096\n65\n", "4095\n65\n", 1),
        "zz": "4096\n65\n" + srs_raw[:48].hex() + "\nzz\n",
        # and: nothing at all; the end of the file inside a hex line; a G2 point whose second coordinate is p or more (only the first
        # one carries flag bits); a monomial G1 line that says infinity and carries a payload (the Lagrange section would take it:
        # those points are decompressed later)
        "empty": "",
        "ends inside a line": text[:len(head) + 97 * 20 + 50],
        "G2 second coordinate = p": compose(g2_lines=replaced([g2.hex()] * 65, 3, (g2_first + ks.P.to_bytes(48, "big")).hex())),
        "G2 second coordinate with the top bits set": compose(g2_lines=replaced([g2.hex()] * 65, 64, (g2_first + b"\xe0" + bytes(47)).hex())),
        "monomial infinity with payload": compose(monomial=replaced(g1_lines, 5, (bytes([0xC0]) + bytes(46) + b"\x01").hex())),
    }
    assert cases["no monomial section"] == "4096\n65\n" + "\n".join(g1_lines) + "\n" + "\n".join([g2.hex()] * 65) + "\n"
    assert len(cases) == 13 and all(body != text for body in cases.values())
    bad = tmp_path / "bad.txt"
    for what, body in cases.items():
        bad.write_text(body)
        assert harness("srs", str(bad)) == invalid, what
    # the counterpart of the last two: the same changes within the rules are accepted
    bad.write_text(compose(g2_lines=replaced([g2.hex()] * 65, 3, (g2_first + (ks.P - 1).to_bytes(48, "big")).hex()),
                           monomial=replaced(g1_lines, 5, (bytes([0xC0]) + bytes(47)).hex())))
    assert harness("srs", str(bad)) == status[cttEthTrustedSetupStatus.cttEthTS_Success] + srs_raw


# ---- EIP-2537 ---------------------------------------------------------------------------------------------------------------------
def _evm_expect(group, raw):
    """-> (parse[] status values, pts bytes, coefs bytes) of the input's pairs, derived in Python integers"""
    ncoord = 2 if group == "g1" else 4
    rec_len = 64 * ncoord + 32
    parse, pts, coefs = [], b"", b""
    for i in range(len(raw) // rec_len):
        rec = raw[i * rec_len:(i + 1) * rec_len]
        chunks = [rec[64 * j:64 * j + 64] for j in range(ncoord)]
        cs = [int.from_bytes(c, "big") for c in chunks]
        pt = bytes(48 * ncoord)
        if any(any(c[:16]) or v >= ks.P for c, v in zip(chunks, cs)):
            st = CttEVMStatus.cttEVM_IntLargerThanModulus
        elif not any(cs):
            st = CttEVMStatus.cttEVM_Success          # the neutral
        elif group == "g1":
            on = (cs[1] * cs[1] - cs[0] ** 3 - 4) % ks.P == 0
            st = CttEVMStatus.cttEVM_Success if on else CttEVMStatus.cttEVM_PointNotOnCurve
            if on:
                pt = ks.aff_mont_bytes((cs[0], cs[1]))
        else:
            Q = ((cs[0], cs[1]), (cs[2], cs[3]))
            on = G2.is_on_curve(Q)
            st = CttEVMStatus.cttEVM_Success if on else CttEVMStatus.cttEVM_PointNotOnCurve
            if on:
                pt = G2.F.to_mont_bytes(Q[0]) + G2.F.to_mont_bytes(Q[1])
        parse.append(st.value)
        pts += pt
        coefs += (int.from_bytes(rec[64 * ncoord:], "big") % ks.R).to_bytes(32, "little")
    return parse, pts, coefs


def _evm_run(harness, group, raw):
    """-> None for an input the length check refuses, else what _evm_expect returns"""
    ncoord = 2 if group == "g1" else 4
    out = harness("evm", group, data=raw)
    if out == bytes([CttEVMStatus.cttEVM_InvalidInputSize.value]):
        return None
    n = len(raw) // (64 * ncoord + 32)
    assert out[0] == CttEVMStatus.cttEVM_Success.value and len(out) == 1 + n * (1 + 48 * ncoord + 32)
    return list(out[1:1 + n]), out[1 + n:1 + n + 48 * ncoord * n], out[1 + n + 48 * ncoord * n:]


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_evm_parser_on_the_reference_vectors(harness, group):
    rec_len = 160 if group == "g1" else 288
    seen = set()
    vectors = [(name, inp) for name, inp, _ in EVM_DOC[group] + EVM_DOC[group + "_fail"]]
    assert len(vectors) >= 20
    for name, inp in vectors:
        raw = bytes.fromhex(inp)
        got = _evm_run(harness, group, raw)
        if len(raw) == 0 or len(raw) % rec_len:
            assert got is None, name
            continue
        want = _evm_expect(group, raw)
        assert got == want, name
        seen |= set(want[0])
    assert seen == {CttEVMStatus.cttEVM_Success.value, CttEVMStatus.cttEVM_IntLargerThanModulus.value,
                    CttEVMStatus.cttEVM_PointNotOnCurve.value}


def test_evm_parser_verdicts_pair_by_pair(harness):
    """the seven inputs of test_status_is_that_of_the_first_offending_point: parse[] holds every pair's own verdict (a point outside
    the subgroup is on the curve: the parser accepts it, the subgroup check is the GPU side's)"""
    sub = next(inp for _, inp, err in EVM_DOC["g1_fail"] if "subgroup" in err)
    off_subgroup = bytes.fromhex(sub)[:128]
    off_curve = (1).to_bytes(64, "big") + (1).to_bytes(64, "big")
    good = bytes.fromhex(EVM_DOC["g1"][0][1])[:128]
    k = (5).to_bytes(32, "big")
    too_large = b"\x00" * 16 + b"\xff" * 48 + (1).to_bytes(64, "big")
    S, L, C = (CttEVMStatus.cttEVM_Success.value, CttEVMStatus.cttEVM_IntLargerThanModulus.value, CttEVMStatus.cttEVM_PointNotOnCurve.value)
    for pts, verdicts in (((off_subgroup, off_curve), [S, C]),
                          ((good, off_curve, too_large), [S, C, L]),
                          ((good, off_subgroup, too_large), [S, S, L]),
                          ((good, too_large, off_curve, off_subgroup), [S, L, C, S]),
                          ((good, off_curve, off_subgroup), [S, C, S]),
                          ((good, good, off_subgroup, off_curve), [S, S, S, C]),
                          ((off_curve, off_subgroup), [C, S])):
        raw = b"".join(p + k for p in pts)
        want = _evm_expect("g1", raw)
        assert want[0] == verdicts
        assert _evm_run(harness, "g1", raw) == want


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_evm_output_encoder(harness, group):
    ncoord = 2 if group == "g1" else 4
    results = [bytes.fromhex(exp) for _, _, exp in EVM_DOC[group]]
    picked = [r for r in results if any(r)][:3] + [bytes(64 * ncoord)]      # three points and the neutral
    assert len(picked) == 4
    for exp in picked:
        cs = [int.from_bytes(exp[64 * j:64 * j + 64], "big") for j in range(ncoord)]
        aff = b"".join((c * ks.MONT % ks.P).to_bytes(48, "little") for c in cs)
        assert harness("evm-out", group, data=aff) == b"".join(c.to_bytes(64, "big") for c in cs) == exp


# ---- EIP-7594 ---------------------------------------------------------------------------------------------------------------------
def test_cell_quotient_body_lane_by_lane(harness):
    """cell_quotient_body over all 8192 lanes against tests/_peerdasref.py, all 128 x 4096 coefficients: the comparison
    test_cell_quotients_kernel makes on the device, here also on a blob of all r - 1"""
    from tests import _peerdasref as pr
    valid_2 = next(blob for case, blob, dig, _ in pr.fixture_cases() if dig is not None and case.endswith("valid_2"))
    for blob in (valid_2, (ks.R - 1).to_bytes(32, "big") * 4096):
        p = pr.coefficients(blob)
        out = harness("cellq", data=b"".join(v.to_bytes(32, "little") for v in p))
        got = np.frombuffer(out, dtype=np.uint8).reshape(pr.CELLS, pr.N, 32)
        assert np.array_equal(got, pr.quotients_array(p))
