"""The checker of tests/test_gpu_slices.py on fabricated buffers (tests/slice_ref.py): one stray element in each region it must
tell apart, found and named; an untouched buffer gives none; the slice comes back converted as layer_debug converts it."""
import numpy as np
import pytest

import oracle_lib as orc
import slice_ref

B, HO, WO, C, LD, CO_OFF, GUARD = 2, 3, 5, 8, 24, 8, 256           # the slice is channels [8, 16) of a 24-wide pixel


def _buffer(es, kind, seed=0):
    """a poisoned allocation whose slice holds finite values; returns (raw bytes, the values written)"""
    ut = np.uint32 if es == 4 else np.uint16
    npix = B * HO * WO
    el = np.full(2 * GUARD // es + npix * LD, np.iinfo(ut).max, ut)
    vals = np.random.default_rng(seed).standard_normal((npix, C)).astype(np.float32)
    if es == 2:
        vals = (orc.bf16_round if kind == 1 else orc.fp16_round)(vals)
        bits = vals.astype(np.float16).view(np.uint16) if kind == 2 else (vals.view(np.uint32) >> 16).astype(np.uint16)
    else:
        bits = vals.view(np.uint32)
    g = GUARD // es
    el[g:g + npix * LD].reshape(npix, LD)[:, CO_OFF:CO_OFF + C] = bits
    return el, vals.reshape(B, HO, WO, C)


def _check(el, es, kind, **kw):
    return slice_ref.check(el.view(np.uint8), es, (B, HO, WO), C, LD, CO_OFF, GUARD, kind, **kw)


KINDS = [(4, 0), (2, 1), (2, 2)]


@pytest.mark.parametrize("es,kind", KINDS)
def test_untouched_buffer_has_no_stray_and_the_slice_comes_back(es, kind):
    el, vals = _buffer(es, kind)
    r = _check(el, es, kind)
    assert r.strays == [] and r.n_strays == 0 and r.unwritten == 0
    assert r.dense.dtype == np.float32 and np.array_equal(r.dense, vals)
    assert slice_ref.describe(r.strays, r.n_strays) == "no stray element"


@pytest.mark.parametrize("es,kind", KINDS)
def test_unwritten_slice_elements_are_counted(es, kind):
    el, _ = _buffer(es, kind)
    g = GUARD // es
    el[g + 7 * LD + CO_OFF + 3] = np.iinfo(el.dtype).max
    el[g + 29 * LD + CO_OFF + C - 1] = np.iinfo(el.dtype).max
    r = _check(el, es, kind)
    assert r.unwritten == 2 and r.n_strays == 0
    assert np.isnan(r.dense[0, 1, 2, 3]) and np.isnan(r.dense[1, 2, 4, C - 1]) and np.count_nonzero(np.isnan(r.dense)) == 2


# (region, element offset from the start of the image region or of the guard) -> the Stray it must give
def _cases(es):
    g, n = GUARD // es, B * HO * WO * LD
    pix = (1 * HO * WO + 2 * WO + 3)                                   # image 1, y 2, x 3
    last = B * HO * WO - 1
    return [
        ("front guard: its first element", 0, ("front guard", 0, None, None, None, None)),
        ("front guard: the element in front of the tensor", g - 1, ("front guard", g - 1, None, None, None, None)),
        ("the gap in front of co_off", g + pix * LD + CO_OFF - 1, ("image", pix * LD + CO_OFF - 1, 1, 2, 3, CO_OFF - 1)),
        ("the first pixel's gap in front of co_off", g, ("image", 0, 0, 0, 0, 0)),
        ("the gap behind co_off + Cout", g + pix * LD + CO_OFF + C, ("image", pix * LD + CO_OFF + C, 1, 2, 3, CO_OFF + C)),
        ("the last pixel's gap", g + last * LD + LD - 1, ("image", last * LD + LD - 1, B - 1, HO - 1, WO - 1, LD - 1)),
        ("back guard: the element behind the tensor", g + n, ("back guard", 0, None, None, None, None)),
        ("back guard: its last element", g + n + g - 1, ("back guard", g - 1, None, None, None, None)),
    ]


@pytest.mark.parametrize("es,kind", KINDS)
@pytest.mark.parametrize("case", range(8))
def test_one_stray_element_in_each_region_is_found_and_named(es, kind, case):
    what, at, want = _cases(es)[case]
    el, vals = _buffer(es, kind)
    value = 1.5                                                         # exact in all three formats
    el[at] = {(4, 0): 0x3FC00000, (2, 1): 0x3FC0, (2, 2): 0x3E00}[(es, kind)]
    r = _check(el, es, kind)
    assert r.n_strays == 1 and len(r.strays) == 1, what
    s = r.strays[0]
    assert (s.region, s.index, s.b, s.y, s.x, s.c) == want, what
    assert s.value == value and s.bits == int(el[at])
    assert r.unwritten == 0 and np.array_equal(r.dense, vals)           # the slice itself is untouched by a stray outside it
    msg = slice_ref.describe(r.strays, r.n_strays)
    assert msg.startswith("1 stray element(s): ") and "1.5" in msg
    assert ("channel=%d" % want[5] in msg) if want[0] == "image" else (want[0] in msg)


def test_a_stray_whose_bytes_are_partly_poison_is_still_found():
    """a 2-byte store into a 4-byte element's upper or lower half changes the element"""
    el, _ = _buffer(4, 0)
    el[3] = 0xFFFF0000
    el[5] = 0x0000FFFF
    r = _check(el, 4, 0)
    assert r.n_strays == 2 and [s.index for s in r.strays] == [3, 5]
    assert r.summary == {"front guard": 2, "back guard": 0, "image": 0}


def test_many_strays_are_counted_and_the_list_is_capped_in_address_order():
    el, _ = _buffer(2, 1)
    g = GUARD // 2
    el[g:g + 30 * LD].reshape(30, LD)[:, CO_OFF + C] = 0x3F80        # every pixel's store one channel too wide
    r = _check(el, 2, 1, limit=4)
    assert r.n_strays == 30 and len(r.strays) == 4
    assert [(s.b, s.y, s.x, s.c) for s in r.strays] == [(0, 0, 0, 16), (0, 0, 1, 16), (0, 0, 2, 16), (0, 0, 3, 16)]
    assert slice_ref.describe(r.strays, r.n_strays).endswith(" ...")
    assert r.summary == {"front guard": 0, "back guard": 0, "image": 30, "channels": (16, 16), "pixels": 30}
    assert "channels 16..16 of 30 pixel(s)" in slice_ref.describe(r.strays, r.n_strays, r.summary)


def test_a_buffer_of_the_wrong_size_is_refused():
    el, _ = _buffer(4, 0)
    with pytest.raises(AssertionError):
        slice_ref.check(el.view(np.uint8)[:-4], 4, (B, HO, WO), C, LD, CO_OFF, GUARD, 0)
