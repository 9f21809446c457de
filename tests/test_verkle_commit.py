"""Batched Verkle commitments without a GPU: the bodies of csrc/verkle_bodies.h (table, commit lane, the tree through its slots, finish)
and ed_madd_pre of csrc/ec.h compiled for the CPU (tests/verkle_harness.cpp) and run lane by lane against the Python-integer oracle and the reference's vectors, and the wiring of the new C ABI
(include/ctt_msm_hip.h part 4) on a box without a device."""
import ctypes
import json
import os
import random
import struct

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests._verkle import build_harness, crafted_triples, expected_finish, fr_from, layout, map_fr, rec_bytes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("verkle"))


@pytest.fixture(scope="module")
def verkle_golden():
    return json.load(open(os.path.join(GOLDEN, "banderwagon_verkle.json")))


@pytest.fixture(scope="module")
def map_golden():
    return json.load(open(os.path.join(GOLDEN, "banderwagon_map_to_field.json")))


def ext_point(b):
    x, y, z, t = (bw.fp_from(b[32 * i:32 * i + 32]) for i in range(4))
    iz = bw.inv(z)
    assert z != 0 and t * z % bw.P == x * y % bw.P     # T = XY/Z
    return (x * iz % bw.P, y * iz % bw.P)


def split_outputs(out, m):
    prj, ser, fr = out[:96 * m], out[96 * m:128 * m], out[128 * m:160 * m]
    assert len(out) == 160 * m
    return ([prj[96 * i:96 * i + 96] for i in range(m)], [ser[32 * i:32 * i + 32] for i in range(m)],
            [fr[32 * i:32 * i + 32] for i in range(m)])


@pytest.mark.parametrize("c", [2, 5, 8])
def test_table_records(harness, c):
    rng = random.Random(c)
    pts = [bw.mul(rng.randrange(bw.R), bw.G), bw.crs(1)[0], bw.add(bw.mul(rng.randrange(bw.R), bw.G), bw.T2)]
    out = harness("table", struct.pack("<II", 3, c) + b"".join(bw.aff_bytes(p) for p in pts))
    lay = layout(c)
    W, rows = struct.unpack("<II", out[:8])
    tab = out[8:]
    assert W == len(lay) and rows == sum(1 << (wd - 1) for _, wd in lay) and len(tab) == 3 * rows * 96
    for i, p in enumerate(pts):
        row = 0
        for w, (off, wd) in enumerate(lay):
            half = 1 << (wd - 1)
            js = {1, half} | ({2, half - 1, rng.randrange(1, half + 1)} if w in (0, 1, W // 2, W - 2, W - 1) else set())
            for j in sorted(j for j in js if 1 <= j <= half):
                e = i * rows + row + j - 1
                assert tab[96 * e:96 * e + 96] == rec_bytes(bw.msm_fast([j << off], [p])), (i, w, j)
            row += half


def test_table_of_neutral_and_order_two(harness):
    out = harness("table", struct.pack("<II", 2, 5) + bw.aff_bytes(bw.O) + bw.aff_bytes(bw.T2))
    W, rows = struct.unpack("<II", out[:8])
    tab = out[8:]
    for e in range(rows):
        assert tab[96 * e:96 * e + 96] == rec_bytes(bw.O)
    row = 0
    for off, wd in layout(5):
        for j in range(1, (1 << (wd - 1)) + 1):
            e = rows + row + j - 1
            assert tab[96 * e:96 * e + 96] == rec_bytes(bw.T2 if (j << off) & 1 else bw.O), (off, j)
        row += 1 << (wd - 1)


def test_ed_madd_pre(harness):
    rng = random.Random(11)
    P, Q = bw.mul(rng.randrange(bw.R), bw.G), bw.mul(rng.randrange(bw.R), bw.G)
    seqs = [[P, P, Q], [P, bw.neg(P), Q, bw.neg(Q)], [bw.O, P, bw.O], [bw.T2, P, bw.T2, bw.T2], [P, bw.O, bw.T2, bw.neg(P)],
            [bw.add(P, bw.T2), P, Q], [bw.G] + [bw.mul(rng.randrange(bw.R), bw.G) for _ in range(6)]]
    for seq in seqs:
        out = harness("madd", struct.pack("<I", len(seq)) + b"".join(rec_bytes(p) for p in seq))
        assert len(out) == 128 * len(seq)
        total = bw.O
        for i, p in enumerate(seq):
            total = bw.add(total, p)
            assert ext_point(out[128 * i:128 * i + 128]) == total, (seq, i)   # (Z != 0 throughout: P + (-P) is (0 : c : c : 0))


# --- the tree through its slots -------------------------------------------------------------------------------------------------------
TREE_GUARD = bytes.fromhex("dec0dec0") * 64      # the harness's sentinel words in front of and behind the stand-in for LDS


def _tree(harness, slots, lanes, first, groups):
    """groups: per group a list of `lanes` entries, None (the in-memory neutral, all zero) or (scalar, z): [scalar]G scaled by z
    -> lane 0 of every group after the tree (128 bytes each)"""
    data = struct.pack("<4I", slots, len(groups), lanes, first)
    for grp in groups:
        assert len(grp) == lanes
        for ent in grp:
            if ent is None:
                data += bytes(128)
            else:
                x, y = bw.msm_fast([ent[0]], [bw.G])
                z = ent[1]
                data += b"".join(bw.fp_bytes(v) for v in (x * z % bw.P, y * z % bw.P, z, x * y * z % bw.P))
    out = harness("tree", data)
    n = len(groups)
    assert len(out) == 128 * n + 512
    assert out[128 * n:128 * n + 256] == TREE_GUARD and out[128 * n + 256:] == TREE_GUARD     # nothing written outside the slots
    return [out[128 * g:128 * g + 128] for g in range(n)]


def _tree_groups(rng, n_groups, lanes, offset=0):
    """lane l of group g holds [1000 g + l + 1 + offset]G with a random Z; a few lanes (lane 0 of group 0 among them) the neutral"""
    return [[None if (7 * l + g) % 13 == 0 else (1000 * g + l + 1 + offset, rng.randrange(1, bw.P)) for l in range(lanes)]
            for g in range(n_groups)]


def _tree_expect(grp, first):
    """the sum of the lanes the tree reaches from level `first`: those below 2 * first (lane 0 alone when the loop does not run)"""
    return bw.msm_fast([sum(ent[0] for ent in grp[:max(1, 2 * first)] if ent is not None) % bw.R], [bw.G])


def _tree_point(b):
    return bw.O if b[64:96] == bytes(32) else ext_point(b)


@pytest.mark.parametrize("slots,lanes,first,n_groups", [(128, 256, 0, 1), (128, 256, 1, 1), (128, 256, 4, 1), (128, 256, 128, 1), (32, 64, 32, 4)])
def test_tree_through_its_slots(harness, slots, lanes, first, n_groups):
    """vk_tree_put / vk_tree_take as k_vk_commit (128 slots, first level live / 2 for n = 1, 2, 8, 256) and k_vk_update (32 slots per
    wave, four waves) run them.  Every lane holds a point, also those the tree must not reach."""
    groups = _tree_groups(random.Random(slots + first), n_groups, lanes)
    if first == 0:
        groups[0][0] = (1, 3)                                 # (n = 1: lane 0 keeps what it has, whatever it is)
    got = _tree(harness, slots, lanes, first, groups)
    for g, grp in enumerate(groups):
        assert _tree_point(got[g]) == _tree_expect(grp, first), g
    # no group's result depends on another group's points: the last group's inputs changed, the others bit for bit as before
    changed = groups[:-1] + _tree_groups(random.Random(99), n_groups, lanes, offset=500)[-1:]
    again = _tree(harness, slots, lanes, first, changed)
    assert again[:-1] == got[:-1]
    assert _tree_point(again[-1]) == _tree_expect(changed[-1], first)
    if n_groups > 1:
        assert again[-1] != got[-1]
        changed = _tree_groups(random.Random(98), n_groups, lanes, offset=700)[:1] + groups[1:]
        assert _tree(harness, slots, lanes, first, changed)[1:] == got[1:]


def _commit(harness, pts, rows, c, fr=False):
    enc = bw.fr_bytes if fr else bw.big_bytes
    data = struct.pack("<IIII", len(pts), c, 1 if fr else 0, len(rows)) + b"".join(bw.aff_bytes(p) for p in pts)
    return split_outputs(harness("commit", data + b"".join(enc(k) for row in rows for k in row)), len(rows))


def test_full_commitment_matches_the_reference(harness, verkle_golden):
    crs = bw.crs(256)
    scalars = [int(h, 16) for h in verkle_golden["commit_scalars"]]
    prj, ser, fr = _commit(harness, crs, [scalars], 8)
    assert "0x" + ser[0].hex() == verkle_golden["commitment"]
    expect = bw.msm_fast(scalars, crs)
    assert bw.fp_from(prj[0][64:]) == 1 and bw.aff_from(prj[0][:64]) == expect
    assert fr_from(fr[0]) == map_fr(expect)


@pytest.mark.parametrize("c", [2, 7, 10])
def test_commit_digits_small_basis(harness, c):
    rng = random.Random(100 + c)
    pts = [bw.mul(rng.randrange(1, bw.R), bw.G) for _ in range(4)] + [bw.T2]
    top = (1 << 253) - 1
    rows = [[0] * 5, [1, 0, 0, 0, 0], [0, 0, 0, 0, 1], [bw.R - 1, bw.R, bw.R + 1, top, 1],
            [int.from_bytes(b"\x80" * 32, "little") & top] * 5, [top] * 5, [rng.randrange(1 << 253) for _ in range(5)], [7, 7, 0, 0, 0]]
    prj, ser, fr = _commit(harness, pts, rows, c)
    for i, row in enumerate(rows):
        expect = bw.msm_fast([k % (2 * bw.R) for k in row], pts)
        assert bw.fp_from(prj[i][64:]) == 1 and bw.aff_from(prj[i][:64]) == expect, i
        # the serialisation identifies (x, y) with (-x, -y); the oracle's neutral test is (0, 1) only
        want = bw.serialize(expect) if expect != bw.T2 else bytes(32)
        assert ser[i] == want and fr_from(fr[i]) == map_fr(expect), i
    frrows = [[k % bw.R for k in row] for row in rows[3:7]]
    prj2, _, _ = _commit(harness, pts, frrows, c, fr=True)
    for i, row in enumerate(frrows):
        assert bw.aff_from(prj2[i][:64]) == bw.msm_fast(row, pts), i


def _finish(harness, triples, K, mask=7):
    data = struct.pack("<III", len(triples), K, mask) + b"".join(bw.fp_bytes(v) for tr in triples for v in tr)
    return split_outputs(harness("finish", data), len(triples))


@pytest.mark.parametrize("K", [1, 7, 8, 9, 64])
def test_finish_on_crafted_triples(harness, K):
    triples = crafted_triples()
    assert len(triples) == 55
    rng = random.Random(K)
    lam = rng.randrange(1, bw.P)
    # a zero Y and a zero Z in the middle of a chunk (and next to each other at a chunk boundary for K = 8, 9)
    triples[3] = (5 * lam % bw.P, 0, lam)
    triples[12] = (7, 9, 0)
    triples[16] = (0, 0, 0)
    triples[17] = (3, 0, 1)
    prj, ser, fr = _finish(harness, triples, K)
    for i, tr in enumerate(triples):
        eprj, eser, efr = expected_finish(tr)
        assert prj[i] == eprj and ser[i] == eser and fr_from(fr[i]) == efr, (K, i)
    assert fr_from(fr[3]) == 0 and ser[12] == bytes(32) and prj[12] == bytes(64) + bw.fp_bytes(1) and fr_from(fr[12]) == 7 * bw.inv(9) % bw.P % bw.R


@pytest.mark.parametrize("m", [1, 7, 8, 9, 16])
def test_finish_chunk_edges_and_output_subsets(harness, m):
    triples = crafted_triples()[20:20 + m]
    full = _finish(harness, triples, 8)
    for i, tr in enumerate(triples):
        eprj, eser, efr = expected_finish(tr)
        assert full[0][i] == eprj and full[1][i] == eser and fr_from(full[2][i]) == efr
    for mask in range(1, 7):
        got = _finish(harness, triples, 8, mask)
        for bit in range(3):
            if mask >> bit & 1:
                assert got[bit] == full[bit], (mask, bit)
            else:
                assert all(b == bytes([0x5A]) * len(b) for b in got[bit]), (mask, bit)


def test_reference_map_and_serialisation_vectors(harness, verkle_golden, map_golden):
    rng = random.Random(3)
    pts, want_fr, want_ser = [], [], []
    for k, h in map_golden["multiples_of_g"]:
        pts.append(bw.mul(k, bw.G))
        want_fr.append(int(h, 16))
        want_ser.append(None)
    for ph, h in map_golden["serialized"]:
        pts.append(bw.deserialize(bytes.fromhex(ph[2:])))
        want_fr.append(int(h, 16))
        want_ser.append(ph)
    assert sum(1 for p in pts if p[0] * bw.inv(p[1]) % bw.P >= bw.R) >= 2      # the reduction mod r is exercised
    pt = bw.G
    for h in verkle_golden["doublings"]:
        pts.append(pt)
        want_fr.append(None)
        want_ser.append(h)
        pt = bw.add(pt, pt)
    triples = []
    for p in pts:
        z = rng.randrange(1, bw.P)
        triples.append((p[0] * z % bw.P, p[1] * z % bw.P, z))
    prj, ser, fr = _finish(harness, triples, 8)
    for i, p in enumerate(pts):
        assert bw.aff_from(prj[i][:64]) == p
        if want_fr[i] is not None:
            assert fr_from(fr[i]) == want_fr[i] == map_fr(p), i
        if want_ser[i] is not None:
            assert "0x" + ser[i].hex() == want_ser[i], i


# --- ABI wiring ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["ctt_hip_verkle_crs_create", "ctt_hip_verkle_crs_destroy", "ctt_hip_verkle_crs_window_bits", "ctt_hip_verkle_commit_batch",
               "ctt_hip_banderwagon_map_to_fr_batch", "ctt_hip_banderwagon_serialize_batch"]


def test_new_symbols_are_exported_and_versioned():
    from constantine_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.exported_symbols() and hasattr(L, s), s
    assert L.ctt_hip_msm_abi_version() == _lib.ABI_VERSION == 11
    assert L.ctt_hip_verkle_crs_window_bits(None) == -1


def test_without_a_device_the_new_symbols_refuse():
    from constantine_amd import _lib
    L = _lib.lib()
    if L.ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    vp = ctypes.c_void_p
    pts = np.frombuffer(b"".join(bw.aff_bytes(p) for p in bw.crs(2)), dtype=np.uint8).copy()
    L.ctt_hip_clear_last_error()
    assert L.ctt_hip_verkle_crs_create(None, pts.ctypes.data_as(vp), 2, 0, 0) is None
    assert L.ctt_hip_last_error() == -3
    coefs = np.zeros((1, 2, 32), np.uint8)
    outs = [np.full(n, 0xAB, np.uint8) for n in (96, 32, 32)]
    o = [a.ctypes.data_as(vp) for a in outs]
    assert L.ctt_hip_verkle_commit_batch(None, None, 0, o[0], o[1], o[2], coefs.ctypes.data_as(vp), 1, 0) == -1
    prj = np.frombuffer(bw.aff_bytes(bw.G) + bw.fp_bytes(1), dtype=np.uint8).copy()
    assert L.ctt_hip_banderwagon_map_to_fr_batch(None, o[2], prj.ctypes.data_as(vp), 1, 0) == -1
    assert L.ctt_hip_last_error() == -3
    assert L.ctt_hip_banderwagon_serialize_batch(None, o[1], prj.ctypes.data_as(vp), 1, 0) == -1
    assert all(bytes(a) == bytes([0xAB]) * len(a) for a in outs)


def test_python_shape_errors_come_before_any_call(monkeypatch):
    from constantine_amd import _lib, verkle

    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded for a call that must be refused in Python")
    monkeypatch.setattr(_lib, "lib", no_gpu)
    with pytest.raises(ValueError):
        verkle.VerkleCrs(np.zeros((3, 63), np.uint8))
    with pytest.raises(ValueError):
        verkle.VerkleCrs(np.zeros((257, 64), np.uint8))
    with pytest.raises(ValueError):
        verkle.VerkleCrs(np.zeros((0, 64), np.uint8))
    with pytest.raises(ValueError):
        verkle.VerkleCrs(np.zeros((4, 64), np.uint8), window_bits=11)
    with pytest.raises(ValueError):
        verkle.batchMapToScalarField(np.zeros((4, 64), np.uint8))
    with pytest.raises(ValueError):
        verkle.serializeBatch_vartime(np.zeros((2, 3, 32), np.uint8))
    crs = verkle.VerkleCrs.__new__(verkle.VerkleCrs)
    crs.n, crs.handle = 4, 1
    with pytest.raises(ValueError):
        crs.commit(np.zeros((2, 5, 32), np.uint8))
    with pytest.raises(ValueError):
        crs.commit(np.zeros((2, 4, 31), np.uint8))
    with pytest.raises(ValueError):
        crs.commit(np.zeros((2, 4, 32), np.uint8), want=())
    with pytest.raises(ValueError):
        crs.commit(np.zeros((2, 4, 32), np.uint8), want=("aff",))


def test_python_refusal_without_a_device():
    from constantine_amd import _lib, verkle
    if _lib.lib().ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    pts = np.frombuffer(b"".join(bw.aff_bytes(p) for p in bw.crs(2)), dtype=np.uint8).reshape(2, 64)
    with pytest.raises(_lib.GpuUnavailable) as e:
        verkle.VerkleCrs(pts)
    assert e.value.code == -3
    with pytest.raises(_lib.GpuUnavailable):
        verkle.batchMapToScalarField(np.zeros((1, 96), np.uint8))
