"""ctt_hip_fr_ntt above n = 4096 on the device, where the width of the index arithmetic shows: 2^13 .. 2^17 compared in full with the
Python integers of tests/_nttref.py (large_cases, shared with the CPU harness test), and 2^20, 2^22, 2^24 and the batch cap of
2^26 elements through the structured references of tests/_nttlarge.py -- sampled outputs of a sparse input, every output of a strided
one, 4096 outputs of a dense one -- with a dense round trip on the device beside them.  Every comparison is equality of 256-bit words.
Inputs are built and outputs gathered on the device; only the few rows compared cross to the host."""
import random

import numpy as np
import pytest

from tests import _nttlarge as big
from tests import _nttref as ref
from tests.test_ntt_gpu import CURVE_OF, _arr, _flags

pytestmark = pytest.mark.gpu

INV, IB, OB = ref.INVERSE, ref.IN_BRP, ref.OUT_BRP
TWO_ADIC = [f for f in ref.FIELDS if ref.large_cases(f)]


def _rows(words):
    import torch
    return torch.from_numpy(_arr(words).reshape(-1, 32)).cuda()


def _index(pos):
    import torch
    return torch.tensor(pos, dtype=torch.int64, device="cuda")


def _shift(p, tag):
    return random.Random("g%s" % (tag,)).randrange(2, p)


def _sparse(plan, p, omega, lg, flags, shift, seed, x=None):
    """(A) on one row: x (n * 32 zero bytes on the device, zero again on return unless the call ran in place)"""
    import torch
    pos_in, val, pos_out, want = big.sparse(p, omega, lg, flags, shift, seed)
    own = x is None
    if own:
        x = torch.zeros(32 << lg, dtype=torch.uint8, device="cuda")
    x.view(-1, 32)[_index(pos_in)] = _rows(val)
    out = torch.empty_like(x)
    plan.ntt(x, shift=shift, out=out, **_flags(flags))
    got = out.view(-1, 32)[_index(pos_out)].cpu().numpy()
    assert ref.from_bytes(got.tobytes()) == want, ("sparse", lg, flags, shift is not None)
    if not own:
        x.view(-1, 32)[_index(pos_in)] = 0


def _strided(plan, p, omega, lg, flags, shift, seed):
    """(B): every output byte, compared on the device"""
    import torch
    pos_in, y, tile, (oshape, tshape) = big.strided(p, omega, lg, flags, shift, seed)
    x = torch.zeros(32 << lg, dtype=torch.uint8, device="cuda")
    x.view(-1, 32)[_index(pos_in)] = _rows(y)
    plan.ntt(x, shift=shift, **_flags(flags))      # in place
    o, t = oshape[:2] + (4,), tshape[:2] + (4,)        # (32 bytes as 4 x int64: an eighth of the comparisons)
    assert bool((x.view(torch.int64).view(*o) == _rows(tile).view(torch.int64).view(*t)).all()), ("strided", lg, flags, shift is not None)


def _dense_input(lg, seed):
    """n words of random bytes below 2^253 on the device"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.randint(0, 256, (1 << lg, 32), dtype=torch.uint8, device="cuda", generator=gen)
    x[:, 31] &= 0x1f
    return x.view(-1)


def _dense(plan, p, omega, lg, flags, x):
    """(C): x is dense; its fold is summed on the host from the bytes the device holds"""
    import torch
    pos_out, want = big.dense(big.fold(x.cpu().numpy(), p, lg, bool(flags & IB)), p, omega, lg, flags)
    out = torch.empty_like(x)
    plan.ntt(x, out=out, **_flags(flags))
    got = out.view(-1, 32)[_index(pos_out)].cpu().numpy()
    assert ref.from_bytes(got.tobytes()) == want, ("dense", lg, flags)


def _round_trip(plan, x, g):
    """(D), a complement to the others: forward to bit-reversed Montgomery residues and back gives the input's bytes"""
    import torch
    y = torch.empty_like(x)
    plan.ntt(x, out=y, shift=g, out_brp=True, out_mont=True)
    assert not torch.equal(y, x)
    plan.ntt(y, inverse=True, in_brp=True, in_mont=True, shift=g)
    assert torch.equal(y, x), "round trip"


@pytest.mark.parametrize("field", TWO_ADIC)
def test_device_matches_python_above_4096(field):
    """tests/_nttref.large_cases: 2^13 .. 2^17 against the full reference"""
    import torch
    from constantine_amd.ntt import NttPlan
    plans = {}
    try:
        for case in ref.large_cases(field):
            name, lg, tile, batch, fl, _sk, in_place = case
            omega, shift, stored, want = ref.large_case_data(field, case)
            if (lg, tile) not in plans:
                plans[(lg, tile)] = NttPlan(CURVE_OF[field], lg, omega, tile_log2=tile)
            plan = plans[(lg, tile)]
            x = _arr(stored)
            t = torch.from_numpy(x).cuda()
            if in_place:
                assert plan.ntt(t, shift=shift, **_flags(fl)) is t
                got = t.cpu().numpy()
            else:
                out = torch.full_like(t, 0xAB)
                plan.ntt(t, shift=shift, out=out, **_flags(fl))
                assert np.array_equal(t.cpu().numpy(), x), (field, name, "the input changed")
                got = out.cpu().numpy()
            assert ref.from_bytes(got.tobytes()) == want, (field, name)
    finally:
        for p in plans.values():
            p.close()


@pytest.mark.parametrize("field", TWO_ADIC)
def test_2p20(field):
    """2^20, a size profiles/ntt.txt times: (A) and (B) on every field, (C) and (D) on BLS12-381 and BN254"""
    from constantine_amd.ntt import NttPlan
    p, lg = ref.FIELDS[field][2], 20
    omega, g = ref.root_of_unity(p, lg), _shift(p, field)
    plan = NttPlan(CURVE_OF[field], lg, omega)
    try:
        assert plan.info()["passes"] == 3
        for flags, shift in ((OB, g), (0, None), (INV | IB, g), (INV, None)):
            _sparse(plan, p, omega, lg, flags, shift, field)
        for flags, shift in ((0, None), (OB, g), (INV | IB, None)):
            _strided(plan, p, omega, lg, flags, shift, field)
        if field in ("bls12_381_fr", "bn254_snarks_fr"):
            x = _dense_input(lg, 20)
            for flags in (OB, INV | IB):
                _dense(plan, p, omega, lg, flags, x)
            _round_trip(plan, x, g)
    finally:
        plan.close()


def test_2p24_bls12_381():
    """2^24, the largest plan there is and the only one with a twiddle exponent bit 22 and a power table entry past 2^23 (the
    inverse shift table has 2^24): (A) with and without shift in both directions, (B), (D)"""
    import torch
    from constantine_amd.ntt import NttPlan
    field, lg = "bls12_381_fr", 24
    p = ref.FIELDS[field][2]
    omega, g = ref.root_of_unity(p, lg), _shift(p, "2p24")
    plan = NttPlan(CURVE_OF[field], lg, omega)
    try:
        x = torch.zeros(32 << lg, dtype=torch.uint8, device="cuda")
        for flags, shift in ((OB, g), (0, None), (INV | IB, g), (INV, None)):
            _sparse(plan, p, omega, lg, flags, shift, "2p24", x)
        del x
        for flags, shift in ((OB, g), (INV | IB, None)):
            _strided(plan, p, omega, lg, flags, shift, "2p24")
        _round_trip(plan, _dense_input(lg, 24), g)
    finally:
        plan.close()


def test_2p24_bn254():
    """(A) on a second field at 2^24, shifted in both directions, and (B) for every output"""
    from constantine_amd.ntt import NttPlan
    field, lg = "bn254_snarks_fr", 24
    p = ref.FIELDS[field][2]
    omega, g = ref.root_of_unity(p, lg), _shift(p, "2p24bn")
    plan = NttPlan(CURVE_OF[field], lg, omega)
    try:
        for flags in (IB | OB, INV):
            _sparse(plan, p, omega, lg, flags, g, "2p24bn")
        _strided(plan, p, omega, lg, 0, None, "2p24bn")
    finally:
        plan.close()


def test_2p24_tile3():
    """eight passes of 2^19 .. 2^21 workgroups, the widest tile indices on both sides of a pass's rows: (A), and (B) for every output"""
    from constantine_amd.ntt import NttPlan
    field, lg = "bls12_381_fr", 24
    p = ref.FIELDS[field][2]
    omega, g = ref.root_of_unity(p, lg), _shift(p, "t3")
    plan = NttPlan(CURVE_OF[field], lg, omega, tile_log2=3)
    try:
        assert plan.info()["passes"] == 8
        _sparse(plan, p, omega, lg, OB, g, "t3")
        _strided(plan, p, omega, lg, INV | IB, None, "t3")
    finally:
        plan.close()


def test_2p22_tile9():
    """the 64 KiB image on a large transform, three passes: (A) in both directions and (B)"""
    from constantine_amd.ntt import NttPlan
    field, lg = "bn254_snarks_fr", 22
    p = ref.FIELDS[field][2]
    omega, g = ref.root_of_unity(p, lg), _shift(p, "t9")
    plan = NttPlan(CURVE_OF[field], lg, omega, tile_log2=9)
    try:
        assert plan.info()["passes"] == 3
        _sparse(plan, p, omega, lg, OB, g, "t9")
        _sparse(plan, p, omega, lg, INV | IB, g, "t9")
        _strided(plan, p, omega, lg, OB, g, "t9")
        _strided(plan, p, omega, lg, INV | IB, None, "t9")
    finally:
        plan.close()


def test_batch_cap_2p13_rows():
    """batch << log2n = 2^26 exactly, 2 GiB in place: 2^13 rows of 2^13, all zero but eight dense ones -- the first, the last, row
    2^12 and five seeded ones -- each compared with the full reference; every other row of the output is zero"""
    import torch
    from constantine_amd.ntt import NttPlan
    field, lg = "bls12_381_fr", 13
    p = ref.FIELDS[field][2]
    n = batch = 1 << lg
    omega, g = ref.root_of_unity(p, lg), _shift(p, "cap13")
    rng = random.Random("cap13")
    rows = {0, batch - 1, 1 << 12}
    while len(rows) < 8:
        rows.add(rng.randrange(1, batch - 1))
    rows = sorted(rows)
    data = {r: ref.stored_inputs(p, n, "cap13 row %d" % r) for r in rows}
    plan = NttPlan(CURVE_OF[field], lg, omega)
    try:
        x = torch.zeros((batch, n * 32), dtype=torch.uint8, device="cuda")
        for r in rows:
            x[r] = _rows(data[r]).view(-1)
        plan.ntt(x.view(-1), shift=g)                         # natural in, natural out: the passes and the swap
        nonzero = x.view(torch.int64).ne(0).any(dim=1).cpu().numpy()
        assert np.flatnonzero(nonzero).tolist() == rows
        for r in rows:
            assert ref.from_bytes(x[r].cpu().numpy().tobytes()) == ref.ntt(data[r], p, omega, shift=g), r
    finally:
        plan.close()


def test_batch_cap_2p24_rows():
    """the same cap as 4 rows of 2^24, in place: (A) on every row, each with its own values"""
    import torch
    from constantine_amd.ntt import NttPlan
    field, lg, batch = "bls12_381_fr", 24, 4
    p = ref.FIELDS[field][2]
    omega, g = ref.root_of_unity(p, lg), _shift(p, "cap24")
    plan = NttPlan(CURVE_OF[field], lg, omega)
    try:
        x = torch.zeros((batch, 32 << lg), dtype=torch.uint8, device="cuda")
        cases = [big.sparse(p, omega, lg, OB, g, "cap24 row %d" % r, samples=500) for r in range(batch)]
        for r, (pos_in, val, _po, _w) in enumerate(cases):
            x[r].view(-1, 32)[_index(pos_in)] = _rows(val)
        plan.ntt(x.view(-1), shift=g, out_brp=True)
        for r, (_pi, _v, pos_out, want) in enumerate(cases):
            got = x[r].view(-1, 32)[_index(pos_out)].cpu().numpy()
            assert ref.from_bytes(got.tobytes()) == want, r
    finally:
        plan.close()
