"""Counter-based random numbers for user kernels: ``pa.random`` (csrc/pk_random.h is the same definition in C++).

``np.random.*`` inside a kernel draws from NumPy's global MT19937 stream, which no parallel engine can reproduce: such a kernel keeps the
host path.  The functions here draw from a STATELESS stream instead -- Philox4x32-10 keyed by (the ParticleSet's ``seed``, the kernel's
position in the list, the ordinal of the draw within the kernel function) and counted by (``particle_id``, the bits of the particle's
``t``) -- so a kernel that uses them compiles into the fused step loop (parcels_amd/jit.py), and the host path, which runs the NumPy
restatement below, gives the same numbers: bit for bit for ``random`` / ``uniform`` / ``integers``, within a few ulp of libm's log / cos for
``normal`` / ``standard_normal`` / ``exponential``.  The numbers of a particle do not depend on the order of the particles, on how an
``execute`` is cut into calls, on the cell sort or on sharding; another ``ParticleSet(seed=)`` gives other numbers.

    def Mortality(particles, fieldset):
        particles.state = np.where(pa.random.random(particles) < fieldset.p_die, StatusCode.Delete, particles.state)

    def RandomWalk(particles, fieldset):
        particles.dx += pa.random.normal(0.0, fieldset.sigma, particles)
        particles.dy += pa.random.normal(0.0, fieldset.sigma, particles)

The LAST positional argument says for whom to draw: the ``particles`` a kernel received, a selection of them (``particles[mask]``: the result
is an array over that selection -- ``random(particles[mask])`` equals ``random(particles)[mask]`` at an equal draw index) or, outside a
kernel, a ``ParticleSet`` (``pa.random.uniform(0.5, 1.5, pset)`` for initial masses: kernel position -1, draw index = the keyword ``stream``;
computed by ``pk_random_fill`` on the device-resident columns when the set is resident, by the restatement otherwise).  Parameters are scalars
or arrays over the same selection; they are taken as float64 (int64 for ``integers``).

Layout (binding; the tests pin it):
  key      k0 = lo32(seed) ^ (0x9E3779B9 * (slot + 1)), k1 = hi32(seed) ^ (0x85EBCA6B * (draw + 1)), products mod 2^32.  k0 is the built-in
           stochastic kernels' (pk_device.h: normal_pair), whose k1 is plain hi32(seed): a user draw never coincides with a built-in one.
  counter  (lo32(id), hi32(id), lo32(tb), hi32(tb)): id = particle_id as uint64, tb = bits of float64(t) + 0.0 (-0.0 and 0.0 are one time)
  rounds   ten, the key bumped by (0x9E3779B9, 0xBB67AE85) behind each -> words w0 .. w3
  uniforms a = w1 << 32 | w0, b = w3 << 32 | w2; u1 = ((a >> 11) + 0.5) * 2^-53, u2 likewise from b: strictly inside (0, 1).  (In float64
           the sum rounds to even; the single value a >> 11 = 2^53 - 1 for which that gives 1.0 takes 1 - 2^-53 instead.)
  random u1 | uniform low + (high - low) * u1 | standard_normal sqrt(-2 log u1) cos(2 pi u2) | normal loc + scale * z |
  exponential scale * (-log u1) | integers low + ((w0 * span) >> 32), span = high - low in [1, 2^32]: value k is too likely by at most
  2^-32, a total bias of at most span / 2^32 (ValueError outside that range).

``draw`` is the number of ``pa.random`` calls the kernel invocation made before this one (host path) = the ordinal of the call site in
source order (compiled): the two agree because the translator refuses a draw that does not execute in every invocation.  A kernel that is
repeated at the same ``t`` (StatusCode.Repeat, AdvectionRK45) draws the same numbers again, as the built-in stochastic kernels do.
"""

from __future__ import annotations

import numpy as np

__all__ = ["random", "uniform", "standard_normal", "normal", "exponential", "integers", "philox4x32", "words", "DrawContext"]

_M32 = np.uint64(0xFFFFFFFF)
_U64 = 0xFFFFFFFFFFFFFFFF
# the codes of pk_random_fill's `dist` (include/parcels_hip.h)
PK_RANDOM_WORDS, PK_RANDOM_RANDOM, PK_RANDOM_UNIFORM, PK_RANDOM_STANDARD_NORMAL, PK_RANDOM_NORMAL, PK_RANDOM_EXPONENTIAL, PK_RANDOM_INTEGERS = range(7)


def philox4x32(counter, key):
    """Ten Philox4x32 rounds.  counter: [..., 4] and key: [..., 2] unsigned 32-bit words (broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter).astype(np.uint64) & _M32
    k = np.asarray(key).astype(np.uint64) & _M32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape) for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape) for j in range(2))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # (32 x 32 bits: exact in uint64)
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & _M32, (p0 >> s) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, slot, draw, ids, t):
    """The four words of every (id, t) pair of the stream (seed, slot, draw): [n, 4] uint32."""
    seed, slot, draw = int(seed) & _U64, int(slot), int(draw)
    if draw < 0:
        raise ValueError(f"draw must not be negative. Got {draw}")
    ids = np.atleast_1d(np.asarray(ids)).astype(np.int64).view(np.uint64)
    tb = (np.atleast_1d(np.asarray(t)).astype(np.float64) + 0.0).view(np.uint64)
    ids, tb = np.broadcast_arrays(ids, tb)
    k0 = (seed & 0xFFFFFFFF) ^ ((0x9E3779B9 * (slot + 1)) & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ ((0x85EBCA6B * (draw + 1)) & 0xFFFFFFFF)
    s = np.uint64(32)
    counter = np.stack([ids & _M32, ids >> s, tb & _M32, tb >> s], axis=-1)
    return philox4x32(counter, np.array([k0, k1], dtype=np.uint64))


def _unit(lo, hi):
    a = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    u = ((a >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    # (the float64 sum rounds to even: a >> 11 = 2^53 - 1 alone would give 1.0; its exact value 1 - 2^-54 takes the lower neighbour instead)
    return np.minimum(u, 1.0 - 2.0**-53)


def _span(low, high):
    """(low as int64 array, span as uint64 array) of integers(low, high); ValueError unless 1 <= span <= 2^32 everywhere."""
    lo, hi = np.asarray(low), np.asarray(high)
    if lo.dtype.kind not in "iub" or hi.dtype.kind not in "iub":
        raise TypeError(f"integers: low and high must be integers. Got {lo.dtype} and {hi.dtype}")
    lo_o, hi_o = lo.astype(object), hi.astype(object)
    span = hi_o - lo_o  # (Python integers: no wrap-around in the test)
    if np.any(span < 1) or np.any(span > 2**32):
        raise ValueError(f"integers(low, high): high - low must lie in [1, 2**32]. Got low={low!r}, high={high!r}")
    return lo.astype(np.int64), np.asarray(span).astype(np.uint64)


def _variates(dist, w, p0=None, p1=None):
    """The variates of the words w [n, 4] (the restatement of csrc/pk_random.h: random_*_of)."""
    if dist == PK_RANDOM_WORDS:
        return w
    if dist == PK_RANDOM_INTEGERS:
        low, span = np.asarray(p0, np.int64).view(np.uint64), np.asarray(p1, np.uint64)  # (w0 * span < 2^64; the sum wraps like int64's)
        return (low + ((w[:, 0].astype(np.uint64) * span) >> np.uint64(32))).view(np.int64)
    u1 = _unit(w[:, 0], w[:, 1])
    if dist == PK_RANDOM_RANDOM:
        return u1
    if dist == PK_RANDOM_UNIFORM:
        return p0 + (p1 - p0) * u1
    if dist == PK_RANDOM_EXPONENTIAL:
        return p0 * (-np.log(u1))
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925286766559 * _unit(w[:, 2], w[:, 3]))
    return z if dist == PK_RANDOM_STANDARD_NORMAL else p0 + p1 * z


class DrawContext:
    """What a kernel invocation on the host path draws with: the set's seed, the kernel's position in the list and the number of draws made so
    far.  hostkernels.execute_hosted makes one per invocation (Repeat re-invocations included); every selection of the view shares it."""

    __slots__ = ("seed", "slot", "draws")

    def __init__(self, seed, slot):
        self.seed, self.slot, self.draws = int(seed) & _U64, int(slot), 0


def _param(v, n, what, dtype=np.float64):
    a = np.asarray(v._parent[v._rows] if hasattr(v, "_parent") else v)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
        raise ValueError(f"{what}: a parameter of shape {a.shape} for {n} particles (parameters are scalars or arrays over the same selection)")
    return a.astype(dtype) if dtype is not None else a


def _draw(who, dist, particles, p0=None, p1=None, stream=None):
    from .hostkernels import HostParticles
    from .particleset import ParticleSet

    if isinstance(particles, HostParticles):
        if stream is not None:
            raise TypeError(f"pa.random.{who}: stream= goes with a ParticleSet; inside a kernel the draw index counts the calls")
        ctx = object.__getattribute__(particles, "_rng")
        if ctx is None:
            raise TypeError(f"pa.random.{who}: these particles carry no draw context (a view made outside Kernel.execute); pass the ParticleSet")
        data, rows = object.__getattribute__(particles, "_data"), object.__getattribute__(particles, "_rows")
        draw, ctx.draws = ctx.draws, ctx.draws + 1
        n = len(rows)
        p0, p1 = _params(who, dist, p0, p1, n)
        return _variates(dist, words(ctx.seed, ctx.slot, draw, np.asarray(data["particle_id"])[rows], np.asarray(data["t"])[rows]), p0, p1)
    if isinstance(particles, ParticleSet):
        draw = 0 if stream is None else int(stream)
        if draw < 0:
            raise ValueError(f"pa.random.{who}: stream must not be negative. Got {stream}")
        n = len(particles)
        p0, p1 = _params(who, dist, p0, p1, n)
        return _draw_for_set(dist, particles, draw, p0, p1)
    raise TypeError(f"pa.random.{who}: the last positional argument must be the particles a kernel received, a selection of them "
                    f"(particles[mask]) or a ParticleSet. Got {type(particles).__name__}")


def _params(who, dist, p0, p1, n):
    if dist == PK_RANDOM_INTEGERS:
        lo, hi = _param(p0, n, who, None), _param(p1, n, who, None)
        return _span(lo, hi)
    return (None if p0 is None else _param(p0, n, who)), (None if p1 is None else _param(p1, n, who))


def _draw_for_set(dist, pset, draw, p0, p1):
    """Outside a kernel: slot -1 (slot + 1 = 0), draw = stream.  On the device-resident columns when the set is resident on an engine
    (pk_random_fill reads particle_id and t where they are, the values come back in row order), by the restatement otherwise."""
    from .columns import LazyColumns, readonly

    data = pset._data
    n = len(pset)
    eng = data._engine if isinstance(data, LazyColumns) and data.resident() else None
    if eng is None or n == 0 or not hasattr(eng, "random_fill"):
        d = readonly(data)
        return _variates(dist, words(pset.seed, -1, draw, np.asarray(d["particle_id"]), np.asarray(d["t"])), p0, p1)
    eng.make_current_for_reading(data)
    # the device computes the variate of scalar parameters; with array parameters it computes the base variate and NumPy applies them (the
    # same roundings: `low + (high - low) * u1`, `loc + scale * z`, `scale * e`)
    scalar = all(p is None or np.ndim(p) == 0 for p in (p0, p1))
    if dist == PK_RANDOM_INTEGERS:
        if scalar:
            return eng.random_fill(dist, pset.seed, -1, draw, ilow=int(p0), span=int(p1))
        w = eng.random_fill(PK_RANDOM_WORDS, pset.seed, -1, draw)
        return _variates(dist, w, p0, p1)
    if scalar:
        return eng.random_fill(dist, pset.seed, -1, draw, p0=0.0 if p0 is None else float(p0), p1=0.0 if p1 is None else float(p1))
    if dist == PK_RANDOM_UNIFORM:
        return p0 + (p1 - p0) * eng.random_fill(PK_RANDOM_RANDOM, pset.seed, -1, draw)
    if dist == PK_RANDOM_EXPONENTIAL:
        return p0 * eng.random_fill(PK_RANDOM_EXPONENTIAL, pset.seed, -1, draw, p0=1.0)
    return p0 + p1 * eng.random_fill(PK_RANDOM_STANDARD_NORMAL, pset.seed, -1, draw)


def random(particles=None, *, stream=None):
    """Uniform on (0, 1), float64: u1 of the layout."""
    return _draw("random", PK_RANDOM_RANDOM, particles, stream=stream)


def uniform(low, high, particles=None, *, stream=None):
    """``low + (high - low) * u1`` in float64 (two roundings behind the difference, no FMA)."""
    return _draw("uniform", PK_RANDOM_UNIFORM, particles, low, high, stream=stream)


def standard_normal(particles=None, *, stream=None):
    """``sqrt(-2 log u1) * cos(2 pi u2)`` (Box-Muller), float64; |z| < 8.66."""
    return _draw("standard_normal", PK_RANDOM_STANDARD_NORMAL, particles, stream=stream)


def normal(loc, scale, particles=None, *, stream=None):
    """``loc + scale * standard_normal`` in float64 (no FMA)."""
    return _draw("normal", PK_RANDOM_NORMAL, particles, loc, scale, stream=stream)


def exponential(scale, particles=None, *, stream=None):
    """``scale * (-log u1)``, float64."""
    return _draw("exponential", PK_RANDOM_EXPONENTIAL, particles, scale, stream=stream)


def integers(low, high, particles=None, *, stream=None):
    """int64 in [low, high): ``low + ((w0 * span) >> 32)`` with ``span = high - low`` in [1, 2**32] (ValueError otherwise) -- a multiply-shift
    in exact integer arithmetic; a value is too likely by at most 2**-32, a total bias of at most ``span / 2**32``."""
    return _draw("integers", PK_RANDOM_INTEGERS, particles, low, high, stream=stream)


_FUNCTIONS = {random: ("random", 0), uniform: ("uniform", 2), standard_normal: ("standard_normal", 0), normal: ("normal", 2),
              exponential: ("exponential", 1), integers: ("integers", 2)}  # function -> (name, number of parameters): what jit.py recognises
