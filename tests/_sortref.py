"""A plain reference of the digit sort (Booth digits + sort by bucket; csrc/hip_backend.hip launch_digits_sort, the contract above
SortArgs in csrc/msm_bodies.h), for tests/test_sort_probe.py.  numpy and Python integers only; nothing of constantine_amd is imported.

A scalar k < 2^bits is cut into W windows over bits + 1 bits whose widths differ by at most one (the first r are cb + 1 bits wide, the
others cb).  The signed digit of window w is  s_w = x_w + b_in - 2^width * b_top  with x_w the window's own bits, b_in the bit below
the window and b_top the window's top bit, so that  sum_w s_w * 2^off(w) == k.  A digit of value val = |s_w| > 0 is a record in bucket
val - 1 of the window's bucket set; its entry is  j | neg << 31  (merged, the window-table form: one set for all windows and the entry
is the table row  (w * id_stride + j) | neg << 31)."""
import numpy as np

DEFAULT_CAP, DEFAULT_BIG = 20480, 1024     # what the probe takes for cap = 0 / big = 0 (msm_plan.h SORT_CAP, SORT_BIG)
FILL = 0xA5                                # the byte the tests pre-fill entries, bstart and the bucket region with
GUARD = 64                                 # guard words behind every output


class WinLayout:
    def __init__(self, bits, c):
        T = bits + 1
        self.W = -(-T // c)
        self.cb = T // self.W
        self.r = T - self.cb * self.W
        self.bits = bits

    def off(self, w):
        return w * self.cb + min(w, self.r)

    def width(self, w):
        return self.cb + (1 if w < self.r else 0)

    def cmax(self):
        return self.cb + (1 if self.r > 0 else 0)

    def is_wide(self, w):
        return self.r == 0 or w < self.r


def window_layout(bits, c):
    return WinLayout(bits, c)


def booth_digit(k, w, lay):
    """(val, neg) of window w of the Python integer k; val == 0: no record."""
    off, cw = lay.off(w), lay.width(w)
    x = (k >> off) & ((1 << cw) - 1)
    b_in = (k >> (off - 1)) & 1 if off > 0 else 0
    b_top = (k >> (off + cw - 1)) & 1
    s = x + b_in - (b_top << cw)
    return abs(s), s < 0


def to_words(ks):
    """Python integers below 2^256 -> (n, 8) uint32, little-endian words (the canonical scalars the sort reads)."""
    raw = b"".join(int(k).to_bytes(32, "little") for k in ks)
    return np.frombuffer(raw, dtype="<u4").reshape(-1, 8).astype(np.uint32)


def from_words(words):
    raw = np.ascontiguousarray(words, dtype="<u4").tobytes()
    return [int.from_bytes(raw[32 * j:32 * j + 32], "little") for j in range(len(raw) // 32)]


def digits(words, lay):
    """val (W, n) int64 and neg (W, n) bool of every window of the (n, 8) uint32 scalars: booth_digit over a bit matrix."""
    words = np.ascontiguousarray(words, dtype="<u4").reshape(-1, 8)
    n = words.shape[0]
    bit = np.zeros((n, 258), dtype=np.int64)         # column i + 1 = bit i of the scalar; column 0 = the bit below bit 0
    bit[:, 1:257] = np.unpackbits(words.view(np.uint8).reshape(n, 32), axis=1, bitorder="little")
    val = np.zeros((lay.W, n), dtype=np.int64)
    neg = np.zeros((lay.W, n), dtype=bool)
    for w in range(lay.W):
        off, cw = lay.off(w), lay.width(w)
        x = bit[:, off + 1:off + 1 + cw] @ (1 << np.arange(cw, dtype=np.int64))
        s = x + bit[:, off] - (bit[:, off + cw] << cw)
        val[w], neg[w] = np.abs(s), s < 0
    return val, neg


def derive(n, bits, c, log2_ng, slice_, merged=0, id_stride=0):
    """The shape the probe derives from its inputs (what it writes to used[]), for an explicit group count and slice."""
    lay = window_layout(bits, c)
    cm = lay.cmax()
    B = 1 << (cm - 1)
    NG = 1 << log2_ng
    gshift = 0
    while (B >> gshift) > NG:
        gshift += 1
    jbits = 0
    if not merged:
        jbits = 1
        while jbits < 31 and (1 << jbits) < n:
            jbits += 1
    return dict(cb=lay.cb, r=lay.r, W=1 if merged else lay.W, Wd=lay.W, B=B, NG=NG, gshift=gshift,
                gshift_narrow=gshift if merged else (gshift - 1 if lay.r > 0 and gshift > 0 else gshift),
                nblk=-(-n // slice_), jbits=jbits, nent=lay.W * n if merged else n)


def expected(words, plan):
    """Per bucket set: counts (B,) int64 and the entries sorted by (bucket, entry) as one uint32 array.  plan: bits, c, and for the
    table form merged = 1 and id_stride."""
    lay = window_layout(plan["bits"], plan["c"])
    B = 1 << (lay.cmax() - 1)
    val, neg = digits(words, lay)
    n = val.shape[1]
    j = np.arange(n, dtype=np.int64)
    sets = []
    if plan.get("merged"):
        rows = (np.arange(lay.W, dtype=np.int64)[:, None] * plan["id_stride"] + j[None, :])
        groups = [(val.ravel(), neg.ravel(), rows.ravel())]
    else:
        groups = [(val[w], neg[w], j) for w in range(lay.W)]
    for v, s, idx in groups:
        keep = v > 0
        assert int(v.max(initial=0)) <= B
        bucket = v[keep] - 1
        entry = idx[keep] | (s[keep].astype(np.int64) << 31)
        order = np.lexsort((entry, bucket))
        sets.append(dict(counts=np.bincount(bucket, minlength=B).astype(np.int64), entries=entry[order].astype(np.uint32)))
    return sets


def group_counts(exp_set, plan_used, wide=True):
    """Records per bucket group of one set: (NG,) int64 (buckets above NG << gshift cannot hold any: asserted)."""
    gs = plan_used["gshift"] if wide else plan_used["gshift_narrow"]
    NG = plan_used["NG"]
    c = exp_set["counts"]
    assert c[NG << gs:].sum() == 0
    return c[:NG << gs].reshape(NG, 1 << gs).sum(axis=1)


def new_outputs(used, zero_bytes):
    """Host images of the four output buffers with their guards, pre-filled the way the tests pre-fill the device buffers."""
    W, B, nent = used["W"], used["B"], used["nent"]
    return dict(entries=np.full(W * nent + GUARD, FILL * 0x01010101, dtype=np.uint32),
                bstart=np.full(W * (B + 1) + GUARD, FILL * 0x01010101, dtype=np.uint32),
                maxcount=np.full(4 + GUARD, 0xFFFFFFFF, dtype=np.uint32),
                buckets=np.full(W * B * zero_bytes + 4 * GUARD, FILL, dtype=np.uint8))


def check_guards(out, used, zero_bytes):
    W, B, nent = used["W"], used["B"], used["nent"]
    word = FILL * 0x01010101
    assert (out["entries"][W * nent:] == word).all(), "guard behind entries"
    assert (out["bstart"][W * (B + 1):] == word).all(), "guard behind bstart"
    assert (out["maxcount"][4:] == 0xFFFFFFFF).all(), "guard behind maxcount"
    assert (out["buckets"][W * B * zero_bytes:] == FILL).all(), "guard behind the bucket region"
    assert len(out["entries"]) == W * nent + GUARD and len(out["bstart"]) == W * (B + 1) + GUARD
    assert len(out["maxcount"]) == 4 + GUARD and len(out["buckets"]) == W * B * zero_bytes + 4 * GUARD


def check(out, exp, used, zero_bytes):
    """Every output of one probe call against expected(): exact integer equality throughout.  `out` as new_outputs() shapes it."""
    W, B, nent = used["W"], used["B"], used["nent"]
    assert len(exp) == W
    check_guards(out, used, zero_bytes)
    word = FILL * 0x01010101
    largest = 0
    for r in range(W):
        counts, want = exp[r]["counts"], exp[r]["entries"]
        bs = out["bstart"][r * (B + 1):(r + 1) * (B + 1)].astype(np.int64)
        ent = out["entries"][r * nent:(r + 1) * nent]
        assert bs[0] == 0, f"set {r}: bstart[0] = {bs[0]}"
        got_counts = np.diff(bs)
        bad = np.nonzero(got_counts != counts)[0]
        assert bad.size == 0, f"set {r}: bucket {bad[0]} holds {got_counts[bad[0]]} entries by bstart, {counts[bad[0]]} expected ({bad.size} buckets differ)"
        total = int(counts.sum())
        assert bs[B] == total == want.size, f"set {r}: bstart[B] = {bs[B]}, {total} non-zero digits"
        bucket = np.repeat(np.arange(B, dtype=np.int64), counts)
        got = ent[:total][np.lexsort((ent[:total], bucket))]       # order inside a bucket is free: sort each bucket's slice
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"set {r}: bucket {bucket[bad[0]]}, position {bad[0] - bs[bucket[bad[0]]]} of its sorted entries: "
                               f"{got[bad[0]]:#x}, expected {want[bad[0]]:#x} ({bad.size} entries differ)")
        tail = np.nonzero(ent[total:] != word)[0]
        assert tail.size == 0, f"set {r}: entries[{total + tail[0]}] beyond bstart[B] was written"
        largest = max(largest, int(counts.max(initial=0)))
        if zero_bytes:
            reg = out["buckets"][r * B * zero_bytes:(r + 1) * B * zero_bytes].reshape(B, zero_bytes)
            empty = counts == 0
            bad = np.nonzero(empty & (reg != 0).any(axis=1))[0]
            assert bad.size == 0, f"set {r}: empty bucket {bad[0]} was not cleared ({bad.size} buckets)"
            bad = np.nonzero(~empty & (reg != FILL).any(axis=1))[0]
            assert bad.size == 0, f"set {r}: non-empty bucket {bad[0]} was touched by the clear ({bad.size} buckets)"
    mc = out["maxcount"]
    assert mc[0] == largest, f"maxcount[0] = {mc[0]}, the largest bucket holds {largest}"
    assert (mc[1:4] == 0).all(), f"maxcount[1..3] = {mc[1:4]}"
