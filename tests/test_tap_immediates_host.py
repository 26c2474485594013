"""The identity behind "conv tap row shifts as LDS immediates" (NOTEBOOK round 6: built, measured, kept in no kernel), on the host.
csrc/conv_dev.h lds_xbase(Pl, h) = Pl * 128 + ((h ^ ((Pl >> 1) & 7)) << 4) is restated here; fragment f is reached by ^ (f << 5).
For a padded-flat pitch P with (P - 1) % 16 == 0 a shift by r map rows is r (P - 1) pixels - whole swizzle periods of 16 pixels - plus
the column-like shift r, so

    lds_xbase(x0 + r P + dx, h) ^ (f << 5)  ==  (lds_xbase(x0 + r + dx, h) ^ (f << 5)) + r (P - 1) 128

and the row term fits a ds_read offset field.  Exhaustive for the pitches of the 16-, 32- and 64-wide maps; false for the pitches of the
8-wide maps and of the 288- and 384-px patch geometries, which is the precondition a launcher would have to test.  Nothing in the tree
uses the identity: the negative result in NOTEBOOK rests on it, and whoever takes tap immediates up again starts from here."""
import numpy as np
import pytest

# (r, dx) as the kernels would use them: rows kernel (P = 65) sets (dx, j) with j = 0..5; wide kernel on 32-wide maps r = mt + ty = 0..5,
# on 16-wide maps r = 2 mt + ty = 0..8; dx = 0..2 everywhere
ROWS = {17: 9, 33: 6, 65: 6}
X0 = np.arange(701).reshape(-1, 1, 1, 1, 1)
H = np.arange(2).reshape(1, -1, 1, 1, 1)
FR = np.arange(4).reshape(1, 1, -1, 1, 1)
DX = np.arange(3).reshape(1, 1, 1, 1, -1)


def lds_xbase(pl, h):
    return pl * 128 + ((h ^ ((pl >> 1) & 7)) << 4)


def pitch_allows_immediates(p):
    return (p - 1) % 16 == 0


def both_sides(p, rows):
    r = np.arange(rows).reshape(1, 1, 1, -1, 1)
    direct = lds_xbase(X0 + r * p + DX, H) ^ (FR << 5)
    by_base = (lds_xbase(X0 + r + DX, H) ^ (FR << 5)) + r * (p - 1) * 128
    return direct, by_base


@pytest.mark.parametrize('p', [17, 33, 65])
def test_row_shift_is_an_immediate(p):
    assert pitch_allows_immediates(p)
    direct, by_base = both_sides(p, ROWS[p])
    assert np.array_equal(direct, by_base)
    assert (ROWS[p] - 1) * (p - 1) * 128 <= 65535              # the largest row term fits the 16-bit offset field
    assert (ROWS[p] - 1) * (p - 1) * 128 == {17: 16384, 33: 20480, 65: 40960}[p]


@pytest.mark.parametrize('p', [9, 10, 19, 25, 37, 73])
def test_other_pitches_keep_the_per_set_form(p):
    assert not pitch_allows_immediates(p)
    direct, by_base = both_sides(p, 6)
    assert np.array_equal(direct[:, :, :, :1], by_base[:, :, :, :1])      # r = 0 is the same expression
    assert not np.array_equal(direct[:, :, :, 1], by_base[:, :, :, 1])    # one map row already moves the swizzle key of some pixel
    for r in range(1, 6):                                                  # exactly the shifts by whole swizzle periods survive
        assert np.array_equal(direct[:, :, :, r], by_base[:, :, :, r]) == (r * (p - 1) % 16 == 0), r
