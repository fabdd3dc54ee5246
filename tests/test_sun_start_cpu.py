"""The row of the sun shadow ray's constants (csrc/vp_device.h sun_row_fill) in numpy binary32, no GPU.

The row holds what start_shadow's general expressions give for a collision point at the origin: far end, squared length, length,
the normalising factor, and the reciprocals of the direction's components (the direction itself is one multiply from the first
and the fourth, and is not stored).  render_k reads a word instead of computing it only where a wave's operands have the bits the
word was computed from, so what has to hold for the change to be sound is exactly this identity; what has to hold for it to PAY on
the sun bench.py renders with is that the squared length does not depend on the collision point inside the box, although the
x component of the difference does."""
import numpy as np
import pytest

import sun_start_cases as SC

f32 = np.float32


def _suns():
    return {"bench": SC.bench_sun(), "oblique": SC.OBLIQUE}


@pytest.mark.parametrize("name", ["bench", "oblique"])
def test_row_is_the_general_form_at_the_origin(name):
    sun = _suns()[name]
    e, d2, ln, r, sd, ir = SC.row(sun)
    assert (e != 0).all()
    for zero in (np.zeros((1, 3), f32), -np.zeros((1, 3), f32)):   # (+0 and -0: a far end without a zero component keeps its bits for both)
        dv, gd2, gln, gr, gsd, gir = SC.general(sun, zero)
        assert np.array_equal(SC.bits(dv[0]), SC.bits(e))
        assert SC.bits(gd2)[0] == SC.bits(d2) and SC.bits(gln)[0] == SC.bits(ln) and SC.bits(gr)[0] == SC.bits(r)
        assert np.array_equal(SC.bits(gsd[0]), SC.bits(sd)) and np.array_equal(SC.bits(gir[0]), SC.bits(ir))
    # the words are finite and the direction is a unit vector to a few ulp
    assert np.isfinite(np.concatenate([e, [d2, ln, r], sd, ir])).all()
    assert abs(float(SC.dot(sd)) - 1.0) < 1e-6
    assert np.allclose(sd, np.asarray(sun, np.float64) / np.linalg.norm(np.asarray(sun, np.float64)), rtol=0, atol=1e-6)


def test_bench_sun_has_a_small_component_and_a_constant_length():
    """sun_dir.x of the baked sun is a rounding residue: the far end's x is about -270, so end.x - ro.x differs for every ro.x -- and
    its square, at most 7.4e4, is absorbed by end.y^2 = 9e19 (ulp 8.8e12): dot(dv, dv) has one bit pattern for |ro.x| <= 1 wherever
    the y and z differences keep the far end's bits (|ro.y| < 512, |ro.z| < 128: half an ulp of end.y and end.z)."""
    sun = SC.bench_sun()
    e, d2, *_ = SC.row(sun)
    assert 100.0 < abs(float(e[0])) < 1000.0 and abs(float(e[1])) > 2.0 ** 33 and 2.0 ** 31 < abs(float(e[2])) < 2.0 ** 32
    rng = np.random.default_rng(11)
    x = np.concatenate([np.linspace(-1.0, 1.0, 4001), rng.uniform(-1.0, 1.0, 4000), [1.0, -1.0, 0.0, -0.0]]).astype(f32)
    ro = np.stack([x, rng.uniform(-1.0, 1.0, x.size).astype(f32), rng.uniform(-1.0, 1.0, x.size).astype(f32)], axis=1)
    dv, gd2, *_ = SC.general(sun, ro)
    assert (SC.bits(gd2) == SC.bits(d2)).all(), "dot(dv, dv) moves inside the default box: the length branch would not fire on the bench"
    assert np.array_equal(SC.bits(dv[:, 1]), np.full(x.size, SC.bits(e[1]))) and np.array_equal(SC.bits(dv[:, 2]), np.full(x.size, SC.bits(e[2])))
    assert len(np.unique(SC.bits(dv[:, 0]))) > 4000, "the x difference should vary: it is why the box-wide certificate never held"
    # so every wave of such origins reads the length, the factor and the y and z reciprocals, and divides for x
    assert (SC.taken(sun, ro) == (1 | 4 | 8)).all()
    # and across the absorption boundaries the operands do move
    far = np.array([[0.0, 513.0, 0.0], [0.0, 0.0, 129.0], [0.0, -600.0, 0.0]], f32)
    dvf, *_ = SC.general(sun, far)
    assert SC.bits(dvf[0, 1]) != SC.bits(e[1]) and SC.bits(dvf[1, 2]) != SC.bits(e[2]) and SC.bits(dvf[2, 1]) != SC.bits(e[1])


def test_oblique_sun_keeps_all_three_axes_inside_the_default_box():
    rng = np.random.default_rng(12)
    ro = rng.uniform(-1.0, 1.0, (4096, 3)).astype(f32)
    assert (SC.taken(SC.OBLIQUE, ro) == 15).all()
