"""Inputs and references of the grid Adam step (csrc/adam.hip, common.hpp: adam_one), no GPU needed.

Three references of ONE step, from the strictest to the most independent:

* ``step32``      adam_one in numpy fp32, operation for operation, from the six fp32 scalars of a table row
                  (miso_adam_scalars_table): what the kernels must give bit for bit.
* ``step64``      the same formula in float64 from the same fp32 inputs and scalars, with a running first-order bound of
                  what an fp32 evaluation at one rounding per operation may differ from it.
* ``step_true64`` torch.optim.Adam's step in float64 from float64 hyper-parameters (oracle.ref_torch.adam6_64 without
                  its shapes): what the operation is meant to be.

``EDGE`` is the table of edge values the three are compared on, ``layout`` puts it into tensors so that every form of
the step (dense float4 / dense scalar / slab / ragged end / flags) meets it.
"""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24                  # unit roundoff of fp32
TINY = 2.0 ** -149              # the smallest subnormal: the absolute error floor of every fp32 operation
CHUNK = 64                      # floats per activity flag (MISO_ADAM_CHUNK)
SLAB = 4 * CHUNK                # floats a wavefront steps at a time

# (lr, beta1, beta2, eps)
HYPERS = ((1e-3, 0.9, 0.999, 1e-8),
          (1e-2, 0.9, 0.99, 1e-15),
          (1.0, 0.0, 0.9, 1e-3),
          (1e-6, 0.5, 0.9999, 1e-8),
          (1e-3, 0.99, 0.9, 1e-8))          # beta1 > beta2
STEPS = (1, 2, 10, 1000, 20000, 1000000)

N_ACTIVE = 256 * 5 + 64 * 2 + 7             # five slabs, two whole chunks of a ragged end, a chunk of seven
N_DENSE = 4 * 300 + 3                       # 300 float4s and a numel % 4 tail of three


def scalars_of(lr, b1, b2, eps, t):
    """The six fp32 scalars of step ``t`` as the library's host code forms them, in Python floats (libm's pow and sqrt
    behind ``**`` and math.sqrt): {1 - b1, b2, 1 - b2, -(lr / (1 - b1^t)), sqrt(1 - b2^t), eps}."""
    bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
    return np.array([1.0 - b1, b2, 1.0 - b2, -(lr / bc1), math.sqrt(bc2), eps], dtype=F32)


def _f32(*xs):
    return tuple(np.ascontiguousarray(x, dtype=F32) for x in xs)


def step32(p, g, m, v, scalars):
    """adam_one (common.hpp) in numpy fp32, one rounding per operation, subnormals kept: -> (p', m', v') fp32.
    The first moment is torch's lerp: m + w (g - m) for w < 0.5, g - (g - m)(1 - w) otherwise."""
    p, g, m, v = _f32(p, g, m, v)
    c1, b2, c2, nss, bc, eps = (F32(s) for s in np.asarray(scalars, dtype=F32))
    with np.errstate(all="ignore"):
        d = g - m
        m2 = m + c1 * d if c1 < F32(0.5) else g - d * (F32(1.0) - c1)
        v2 = v * b2 + (c2 * g) * g
        den = np.sqrt(v2) / bc + eps
        p2 = p + (nss * m2) / den
    assert p2.dtype == m2.dtype == v2.dtype == F32
    return p2, m2, v2


def step64(p, g, m, v, scalars):
    """The formula of step32 in float64 from the same fp32 inputs and scalars -> ((p', m', v'), (e_p, e_m, e_v)).

    e_*: a first-order bound of |fp32 evaluation - float64 value| for an evaluation that rounds once per operation,
    formed beside the value.  Every operation z = x op y adds u |z| (u = 2^-24) for its own rounding and 2^-149 for the
    subnormal floor to what its operands' errors propagate to:
      d = g - m                e_d = u |d|
      t = c1 d                 e_t = c1 e_d + u |t|              (the other lerp form: k = 1 - c1, t = d k,
      m' = m + t               e_m = e_t + u |m'|                 e_t = k e_d + |d| u k + u |t|, m' = g - t)
      a = c2 g, b = a g        e_a = u |a|, e_b = |g| e_a + u |b|
      w = v b2, v' = w + b     e_w = u |w|, e_v = e_w + e_b + u |v'|
      s = sqrt(v')             e_s = e_v / (2 s) + u |s|         (s = 0: sqrt(e_v))
      q = s / bc               e_q = e_s / bc + u |q|
      den = q + eps            e_den = e_q + u |den|
      num = nss m'             e_num = |nss| e_m + u |num|
      r = num / den            e_r = e_num / den + |num| e_den / den^2 + u |r|
      p' = p + r               e_p = e_r + u |p'|
    The three bounds returned are doubled for the second-order terms.  Derived, not measured.  Valid where the fp32
    evaluation stays finite (EDGE_FINITE)."""
    p, g, m, v = (np.asarray(x, dtype=F32).astype(np.float64) for x in (p, g, m, v))
    c1, b2, c2, nss, bc, eps = (float(s) for s in np.asarray(scalars, dtype=F32))
    a_ = np.abs
    with np.errstate(all="ignore"):
        d = g - m
        e_d = U * a_(d) + TINY
        if F32(c1) < F32(0.5):
            t = c1 * d
            e_t = c1 * e_d + U * a_(t) + TINY
            m2 = m + t
        else:
            k = 1.0 - c1                            # exact in fp32 for c1 in [0.5, 1]; u k allowed all the same
            t = d * k
            e_t = k * e_d + a_(d) * (U * k) + U * a_(t) + TINY
            m2 = g - t
        e_m = e_t + U * a_(m2) + TINY
        a = c2 * g
        e_a = U * a_(a) + TINY
        b = a * g
        e_b = a_(g) * e_a + U * a_(b) + TINY
        w = v * b2
        e_w = U * a_(w) + TINY
        v2 = w + b
        e_v = e_w + e_b + U * a_(v2) + TINY
        s = np.sqrt(v2)
        e_s = np.where(s > 0, e_v / (2.0 * np.where(s > 0, s, 1.0)), np.sqrt(e_v)) + U * s + TINY
        q = s / bc
        e_q = e_s / bc + U * a_(q) + TINY
        den = q + eps
        e_den = e_q + U * a_(den) + TINY
        num = nss * m2
        e_num = abs(nss) * e_m + U * a_(num) + TINY
        r = num / den
        e_r = e_num / den + a_(num) * e_den / (den * den) + U * a_(r) + TINY
        p2 = p + r
        e_p = e_r + U * a_(p2) + TINY
    return (p2, m2, v2), (2.0 * e_p, 2.0 * e_m, 2.0 * e_v)


def step_true64(p, g, m, v, t, lr, b1, b2, eps):
    """Step number ``t`` (1-based) of torch.optim.Adam (no amsgrad, no weight decay) in float64 from float64
    hyper-parameters -> (p', m', v', r, q / den): r the update p' - p, q / den = (sqrt(v') / sqrt(bc2)) / denominator,
    the share of the denominator that carries bc2_sqrt's rounding."""
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m2 = b1 * m + (1.0 - b1) * g
        v2 = b2 * v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
        q = np.sqrt(v2) / math.sqrt(bc2)
        den = q + eps
        r = -(lr / bc1) * m2 / den
    return p + r, m2, v2, r, q / den


# ---- the edge table -----------------------------------------------------------------------------------------------------
G_VALUES = _f32([0.0, -0.0, 1.4e-45, -1.4e-45,     # +-0, the smallest subnormal
                 1e-40,                            # a subnormal
                 1e-23, 1e-20,                     # g^2 underflows to 0; c2 g^2 is subnormal
                 1e-10, 1e-8, 1e-6,                # sqrt(v) crosses eps
                 1e-3, 1.0,
                 1e19, 3e19,                       # v near the top of fp32
                 1e25,                             # v overflows to inf
                 np.inf, np.nan])[0]
# reachable (m, v); the last a state with m != 0 = v, which a loaded checkpoint can hold
STATES = _f32([(0.0, 0.0), (1e-3, 1e-6), (-1e-3, 1e-6), (1e-20, 1e-40), (1.0, 3e38), (1e-3, 0.0)])[0]
P_VALUES = _f32([0.0, -0.0, 1.0, -1.0, 1e-30, 3e38])[0]

_REC = np.dtype([("p", F32), ("g", F32), ("m", F32), ("v", F32)])


def _edge():
    gi, si, pi = np.meshgrid(np.arange(len(G_VALUES)), np.arange(len(STATES)), np.arange(len(P_VALUES)), indexing="ij")
    gi, si, pi = gi.ravel(), si.ravel(), pi.ravel()
    order = np.random.default_rng(20).permutation(gi.size)
    gi, si, pi = gi[order], si[order], pi[order]
    rec = np.empty(gi.size, dtype=_REC)
    rec["p"], rec["g"], rec["m"], rec["v"] = P_VALUES[pi], G_VALUES[gi], STATES[si, 0], STATES[si, 1]
    return rec, gi, si


EDGE, EDGE_G_CLASS, EDGE_STATE_CLASS = _edge()
N_CLASSES = len(G_VALUES) * len(STATES)
EDGE_CLASS = EDGE_G_CLASS * len(STATES) + EDGE_STATE_CLASS          # (g value, state) of a record


def _finite_part():
    """The records whose step stays finite in fp32 at every HYPERS x STEPS: no NaN, no inf, neither in the inputs nor
    in v' (which overflows first) nor in the outputs.  Results that underflow -- to a subnormal or to zero -- are part of
    it: the bound's 2^-149 floor is there for them."""
    ok = np.isfinite(EDGE["g"])
    for lr, b1, b2, eps in HYPERS:
        for t in STEPS:
            for out in step32(EDGE["p"], EDGE["g"], EDGE["m"], EDGE["v"], scalars_of(lr, b1, b2, eps, t)):
                ok &= np.isfinite(out)
    return ok


EDGE_FINITE_MASK = _finite_part()
EDGE_FINITE = EDGE[EDGE_FINITE_MASK]


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


def same_by_class(got, want):
    """fp32 arrays equal bit for bit, except that a NaN is matched by any NaN (+-inf have one bit pattern each)."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- layouts ----------------------------------------------------------------------------------------------------------------
# What a chunk of 64 floats holds:
#   E  records of EDGE in turn (every such chunk holds non-zero gradients: it is stepped whatever its flag)
#   S  gradients +0 but for ONE, the subnormal 1e-40: the chunk must wake
#   Z  gradients +0 and -0 only, never stepped: must stay asleep, p / m / v bits unchanged
#   W  as Z but stepped before (active = 1): stepped with a zero gradient, and zero_grad leaves +0 for its -0
ROLES = "EZEWESEEWEZESE"
N_ROT = len(ROLES)


class Layout:
    """n floats of (p, g, m, v), the planted ``active`` flags, and what the step rules make of them."""

    def __init__(self, n, rot, dense=False):
        self.n, self.rot = n, rot
        nch = (n + CHUNK - 1) // CHUNK
        self.nchunks = nch
        # (the dense form steps everything and has no flags: EDGE everywhere)
        role = np.array(["E" if dense else ROLES[(c + rot) % N_ROT] for c in range(nch)])
        role_el = np.repeat(role, CHUNK)[:n]
        idx = np.empty(n, dtype=np.int64)
        is_e = role_el == "E"
        # E chunks take the records in turn from a start that moves with rot; the others take every seventh, so that
        # their p / m / v vary too
        idx[is_e] = (np.arange(int(is_e.sum())) + rot * 97) % EDGE.size
        idx[~is_e] = (np.arange(int((~is_e).sum())) * 7 + rot) % EDGE.size
        # the dense numel % 4 tail: (g value, state) classes in turn, three per rotation
        for j, i in enumerate(range(n - n % 4, n)):
            if role_el[i] == "E":
                idx[i] = int(np.flatnonzero(EDGE_CLASS == (3 * rot + j) * 5 % N_CLASSES)[rot % len(P_VALUES)])
        self.index = idx
        self.role = role
        p, g, m, v = (EDGE[k][idx].copy() for k in ("p", "g", "m", "v"))
        pos = np.arange(n)
        in_chunk = pos % CHUNK
        g[~is_e] = 0.0
        g[(role_el != "E") & (role_el != "S") & (in_chunk % 3 == 1)] = -0.0          # Z and W: some -0
        first = np.flatnonzero(role == "S") * CHUNK                                   # S: one subnormal, lane varies
        lane = np.minimum((first // CHUNK * 5 + rot) % CHUNK, n - 1 - first)
        g[first + lane] = 1e-40
        self.p, self.g, self.m, self.v = p, g, m, v
        # planted flags: every W chunk, and every other E chunk (both the up-front loads and the wake-up branch see EDGE)
        self.active = ((role == "W") | ((role == "E") & (np.arange(nch) % 2 == 1))).astype(np.uint8)
        pad = np.zeros(nch * CHUNK, dtype=bool)
        pad[:n] = bits(g) << 1 != 0                                                   # bits that are not +-0 (NaN counts)
        self.nonzero = pad.reshape(nch, CHUNK).any(1)                                  # = the `touched` flags of the step
        self.stepped = self.nonzero | (self.active != 0)                               # = `active` after the step
        self.stepped_el = np.repeat(self.stepped, CHUNK)[:n]
        self.nonzero_el = np.repeat(self.nonzero, CHUNK)[:n]
        self.slab_el = pos < n // SLAB * SLAB                                          # float4 path of the flag forms
        self.vec_el = pos < n - n % 4                                                  # float4 path of the dense form

    def expect(self, scalars, dense):
        """(p', m', v') fp32 after one step: step32 where the form steps (everywhere for the dense one)."""
        out = step32(self.p, self.g, self.m, self.v, scalars)
        if dense:
            return out
        return tuple(np.where(self.stepped_el, new, old) for new, old in zip(out, (self.p, self.m, self.v)))

    def bound(self, scalars):
        """step64's values and bounds on this layout, and the mask of the elements they hold for: a finite gradient and
        a step that stays finite in fp32 (on the records of EDGE that is EDGE_FINITE or more)."""
        val, err = step64(self.p, self.g, self.m, self.v, scalars)
        ok = np.isfinite(self.g)
        for out in step32(self.p, self.g, self.m, self.v, scalars):
            ok = ok & np.isfinite(out)
        return val, err, ok


def layout(n, rot, dense=False):
    return Layout(n, rot % N_ROT, dense)


def coverage(n, dense):
    """-> {path: set of (g value, state) classes of EDGE that the rotations put on that path}; the paths are the dense
    form's 'vec' / 'tail' or the flag forms' 'slab' / 'ragged'."""
    seen = {}
    for rot in range(N_ROT):
        L = layout(n, rot, dense)
        e = np.repeat(L.role == "E", CHUNK)[:n]
        first = L.vec_el if dense else L.slab_el
        for name, where in ((("vec", "tail") if dense else ("slab", "ragged"))[0], first), \
                           ((("vec", "tail") if dense else ("slab", "ragged"))[1], ~first):
            seen.setdefault(name, set()).update(EDGE_CLASS[L.index[where & e]].tolist())
    return seen
