"""tests/lsm_range_model.py (the reference of tests/test_gpu_lsm_get_edges.py) pinned to the
reference's own expression, ``first_key <= key <= last_key`` on ``str`` (src/lsm_storage.py:173),
and its packers checked against themselves.  No GPU."""
import numpy as np

import lsm_range_model as RM


def test_bytes_order_is_the_reference_str_expression():
    """Over every UTF-8 length boundary (U+0000, U+007F | U+0080, U+07FF | U+0800, U+FFFF |
    U+10000, U+10FFFF; no surrogates), pairs, prefixes and the empty string: the model on the
    UTF-8 bytes equals the reference's expression on the strs, for every (first, last, key)."""
    strs = RM.boundary_strs()
    assert "" in strs and all(chr(c) in strs for c in RM.BOUNDARY_CODE_POINTS) and len(strs) > 80
    assert {len(chr(c).encode()) for c in RM.BOUNDARY_CODE_POINTS} == {1, 2, 3, 4}
    assert any(a != b and b.startswith(a) for a in strs for b in strs)  # proper prefixes
    bounds = [(a, b) for a in strs for b in strs[::3]]
    want = np.array([[first <= key <= last for key in strs] for first, last in bounds])
    enc = [s.encode("utf-8") for s in strs]
    benc = [(a.encode("utf-8"), b.encode("utf-8")) for a, b in bounds]
    got = RM.range_bits(enc, benc)
    assert got.dtype == bool and got.shape == (len(bounds), len(strs))
    assert np.array_equal(got, want)
    assert want.any() and not want.all() and any(a > b for a, b in bounds)
    assert np.array_equal(RM.range_bits_ranked(enc, benc), want)


def test_ranked_form_equals_the_plain_form_on_raw_bytes():
    """Bytes no str encodes to (0x80, 0xFF alone), NUL, duplicates, empty bounds, first > last."""
    pool = [b"", b"\x00", b"\x00\x00", b"\x01", b"\x7f", b"\x80", b"\xff", b"\xff\x00", b"a", b"a\x00", b"a\xff", b"ab"]
    keys = pool + pool[3:7]
    bounds = [(a, b) for a in pool for b in pool]
    assert np.array_equal(RM.range_bits_ranked(keys, bounds), RM.range_bits(keys, bounds))
    bits = RM.range_bits(keys, [(b"\x00", b"\x7f"), (b"\x80", b"\x7f"), (b"", b"")])
    assert bits[0].tolist() == [k != b"" and k <= b"\x7f" for k in keys]  # unsigned bytes, NUL > empty
    assert not bits[1].any() and bits[2].tolist() == [k == b"" for k in keys]


def test_packers_round_trip():
    strings = [b"", b"\x00", b"abc", b"", b"\xff\xfe", b"\x00\x00\x00\x00\x00"]
    buf, offs = RM.pack_strings(strings)
    assert buf.dtype == np.uint8 and offs.dtype == np.uint64 and offs[0] == 0 and offs[-1] == buf.size == 11
    assert RM.unpack_strings(buf, offs) == strings
    wbuf, woffs = RM.pack_strings(strings, prefix=b"head!")
    assert woffs[0] == 5 and bytes(wbuf[:5]) == b"head!" and RM.unpack_strings(wbuf, woffs) == strings
    assert np.array_equal(woffs - woffs[0], offs)
    bounds = [(b"a", b"b"), (b"", b"\xff"), (b"zz", b"")]
    bbuf, boffs = RM.pack_bounds(bounds)
    flat = RM.unpack_strings(bbuf, boffs)
    assert len(boffs) == 2 * len(bounds) + 1 and list(zip(flat[0::2], flat[1::2])) == bounds
    ebuf, eoffs = RM.pack_strings([])
    assert ebuf.size == 0 and eoffs.tolist() == [0]


def test_mask_pack_and_unpack_ignore_and_never_invent_pad_bits():
    rng = np.random.default_rng(11)
    for n in (0, 1, 7, 8, 9, 63, 64, 65):
        bits = rng.random((3, n)) < 0.5
        if n:
            bits[0, n - 1], bits[1, n - 1] = True, False
        m = RM.pack_mask(bits)
        assert m.shape == (3, RM.row_bytes(n)) and m.dtype == np.uint8
        assert np.array_equal(RM.unpack_mask(m, 3, n), bits)
        assert np.array_equal(RM.unpack_mask(m.reshape(-1), 3, n), bits)  # the flat C layout
        if n % 8:
            pad = 0xFF & ~((1 << (n % 8)) - 1)
            assert not (m[:, -1] & pad).any()  # packed: the pad bits are zero
            dirty = m.copy()
            dirty[:, -1] |= pad  # unpacked: set pad bits do not show
            assert np.array_equal(RM.unpack_mask(dirty, 3, n), bits)
            assert not np.array_equal(dirty, RM.pack_mask(bits))  # and a byte compare still sees them
    assert RM.pack_mask(np.array([[True] + [False] * 8])).tolist() == [[1, 0]]  # LSB first
    assert RM.unpack_mask(np.array([0x80, 0x01], np.uint8), 1, 9).tolist() == [[False] * 7 + [True, True]]
