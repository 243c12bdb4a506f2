"""Named volumes for the marching-cubes tests (numpy only, seeded): every builder returns ``(u, iso)`` with ``u``
float32 of shape (nx, ny, nz).  The HIP sweeps work on 64-bit words, one bit per sample along z, so each case is
the smallest volume that reaches one piece of their word logic; tests/test_mcubes.py pins on the CPU that each
still does, then compares the device with the oracle bit for bit."""
import numpy as np

F = np.float32


def _randn(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(F)


# last chunk of a row full / holding one sample; 5, 6 and 11 chunks per row: the sign loop (4 words per trip) makes
# its second and third trips and ends on a partial one
WORD_EDGE_SHAPES = ((2, 2, 64), (2, 2, 65), (3, 5, 128), (3, 5, 129), (5, 4, 257), (3, 3, 321), (2, 3, 700))


def word_edges(shape):
    return _randn(1000 + sum(shape), shape), F(0.05)


# nz == 1 has no cells at all; the others are one cell thick along z, z, x
FLAT_SHAPES = ((9, 7, 1), (7, 6, 2), (70, 3, 3), (2, 9, 2))


def flat(shape):
    return _randn(2000 + sum(shape), shape), F(0.05)


def blocks():
    """513 rows (four rows per block of the sign sweep: the last block holds one) and 513 words (256 words per
    block of the edge sweep: the third block holds one)."""
    return _randn(3000, (19, 27, 5)), F(0.05)


def ties(iso):
    """Integer samples in [-2, 2]: a fifth of them equal iso (0.0 or 1.0) and count as not below; the vertices of
    their edges sit on lattice points (t == 0 or t == 1)."""
    u = np.random.RandomState(4000).randint(-2, 3, size=(9, 8, 130)).astype(F)
    return u, F(iso)


def neg_zero():
    """``ties`` with every 0.0 written as -0.0: -0.0 < 0.0 is false, the mesh is that of ``ties`` at iso 0."""
    u, _ = ties(0.0)
    u = u.copy()
    u[u == 0.0] = F(-0.0)
    assert np.signbit(u[u == 0.0]).all()
    return u, F(0.0)


def checker():
    """Alternating signs: every lattice edge is crossed (all vertex words are all ones up to the row's end, ranks
    run to 63) and every cell has 4 triangles."""
    x, y, z = np.meshgrid(np.arange(5), np.arange(4), np.arange(130), indexing="ij")
    sign = 1.0 - 2.0 * ((x + y + z) % 2)
    return (sign * (1.0 + 0.25 * ((7 * x + 3 * y + z) % 5))).astype(F), F(0.0)


def non_finite():
    """1 % NaN, 1 % +inf, 1 % -inf (one uniform draw per sample decides): NaN and +inf are not below."""
    rs = np.random.RandomState(5000)
    u = rs.standard_normal((8, 9, 131)).astype(F)
    r = rs.uniform(size=u.shape)
    u[r < 0.01] = np.nan
    u[(r >= 0.01) & (r < 0.02)] = np.inf
    u[(r >= 0.02) & (r < 0.03)] = -np.inf
    return u, F(0.05)


def extremes(kind):
    """The crossing formula at the ends of the fp32 range: subnormal samples, and samples whose difference
    ``ub - ua`` overflows."""
    u = _randn(6000, (6, 5, 70))
    scale = {"subnormal": F(2.0) ** F(-140), "huge": F(1e38)}[kind]
    with np.errstate(over="ignore", under="ignore"):
        return (u * scale).astype(F), F(0.0)


def _ones():
    return np.ones((6, 7, 300), dtype=F)


def corner():
    """One sample below, in the last lane of the last word of the last row: 3 vertices, 1 triangle."""
    u = _ones()
    u[5, 6, 299] = -1.0
    return u, F(0.0)


def straddle():
    """Two tiny surfaces whose cells sit on both sides of a word boundary (z = 63 | 64 and z = 191 | 192)."""
    u = _ones()
    u[2, 3, 63] = u[2, 3, 64] = -1.0
    u[3, 3, 191] = -2.0
    return u, F(0.0)


def constant(kind):
    """Nothing crosses (all above), all equal to iso, all below: empty meshes."""
    u = _ones()
    return {"above": (u, F(0.0)), "equal": (u, F(1.0)), "below": (-u, F(0.0))}[kind]


def ellipsoid():
    """A closed surface through all 8 chunks of a 512-sample row."""
    x, y, z = np.meshgrid(np.arange(40.0), np.arange(40.0), np.arange(512.0), indexing="ij")
    u = np.sqrt(((x - 19.3) / 12) ** 2 + ((y - 20.1) / 12) ** 2 + ((z - 255.7) / 240) ** 2) - 1
    return u.astype(F), F(0.0)


SHIFTS = (1, 50, 120, 250, 379)


def shifted(z0):
    """The same (6, 5, 20) noise block at z0 in a volume of ones: across each word boundary, and across the 256
    samples of one trip of the sign loop."""
    u = np.ones((6, 5, 400), dtype=F)
    u[:, :, z0:z0 + 20] = _randn(7000, (6, 5, 20))
    return u, F(0.05)


def _tag(shape):
    return "x".join(str(s) for s in shape)


CASES = {}
CASES.update({f"word_edges-{_tag(s)}": (word_edges, s) for s in WORD_EDGE_SHAPES})
CASES.update({f"flat-{_tag(s)}": (flat, s) for s in FLAT_SHAPES})
CASES["blocks"] = (blocks,)
CASES["ties-iso0"] = (ties, 0.0)
CASES["ties-iso1"] = (ties, 1.0)
CASES["neg_zero"] = (neg_zero,)
CASES["checker"] = (checker,)
CASES["non_finite"] = (non_finite,)
CASES["extremes-subnormal"] = (extremes, "subnormal")
CASES["extremes-huge"] = (extremes, "huge")
CASES["corner"] = (corner,)
CASES["straddle"] = (straddle,)
CASES.update({f"constant-{k}": (constant, k) for k in ("above", "equal", "below")})
CASES["ellipsoid"] = (ellipsoid,)
CASES.update({f"shifted-{z0}": (shifted, z0) for z0 in SHIFTS})


def build(name):
    fn, *args = CASES[name]
    u, iso = fn(*args)
    assert u.dtype == F and u.flags["C_CONTIGUOUS"]
    return u, F(iso)
