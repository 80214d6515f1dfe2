"""Built-in kernels (names and signatures of src/parcels/kernels/_advection.py, _advectiondiffusion.py and _sigmagrids.py).

These functions are *tokens*: ``Kernel`` recognises them by identity (the reference does the same for
AdvectionRK45, kernel.py:129-134) and maps each to the PK_KERNEL_* id of the HIP implementation in
csrc/pk_kernels.h.  Their bodies never run; calling one directly is an error, because this package has no
NumPy execution path.  The interaction kernels AttractTowards / MergeNearest are the exception: their tokens have a real Python body on
the device neighbour search, which the host loop runs when the list does not take the device route (parcels_amd/interactkernels.py).
"""

from __future__ import annotations

__all__ = [
    "AdvectionDiffusionEM",
    "AdvectionDiffusionM1",
    "AdvectionEE",
    "AdvectionRK2",
    "AdvectionRK2_3D",
    "AdvectionRK2_3D_CROCO",
    "AdvectionRK4",
    "AdvectionRK4_3D",
    "AdvectionRK45",
    "AttractTowards",
    "DeleteOutOfBounds",
    "DeleteParticle",
    "DiffusionUniformKh",
    "DoNothing",
    "MergeNearest",
    "MoveEast",
    "MoveNorth",
    "SampleField",
    "SampleFieldCroco",
    "SampleOmegaCroco",
    "SubmergeParticle",
    "convert_z_to_sigma_croco",
]


def _device_only(name):
    raise RuntimeError(
        f"{name} is a device kernel of parcels_amd: pass it to ParticleSet.execute(); it cannot be called on the host"
    )


def AdvectionEE(particles, fieldset):  # _advection.py:78-82
    """Explicit Euler advection."""
    _device_only("AdvectionEE")


def AdvectionRK2(particles, fieldset):  # _advection.py:21-28
    """Second-order Runge-Kutta advection."""
    _device_only("AdvectionRK2")


def AdvectionRK2_3D(particles, fieldset):  # _advection.py:31-39
    """Second-order Runge-Kutta advection including vertical velocity."""
    _device_only("AdvectionRK2_3D")


def AdvectionRK4(particles, fieldset):  # _advection.py:42-55
    """Fourth-order Runge-Kutta advection."""
    _device_only("AdvectionRK4")


def AdvectionRK4_3D(particles, fieldset):  # _advection.py:58-75
    """Fourth-order Runge-Kutta advection including vertical velocity."""
    _device_only("AdvectionRK4_3D")


def AdvectionRK45(particles, fieldset):  # _advection.py:85-155
    """Adaptive Runge-Kutta-Fehlberg 4(5) advection (needs RK45_tol/RK45_min_dt/RK45_max_dt and a next_dt Variable)."""
    _device_only("AdvectionRK45")


def AdvectionDiffusionM1(particles, fieldset):  # _advectiondiffusion.py:21-67
    """2-D advection-diffusion, Milstein scheme of order 1 (needs Kh_zonal, Kh_meridional, fieldset.dres)."""
    _device_only("AdvectionDiffusionM1")


def AdvectionDiffusionEM(particles, fieldset):  # _advectiondiffusion.py:70-117
    """2-D advection-diffusion, Euler-Maruyama scheme."""
    _device_only("AdvectionDiffusionEM")


def DiffusionUniformKh(particles, fieldset):  # _advectiondiffusion.py:120-153
    """2-D diffusion with uniform Kh (no advection)."""
    _device_only("DiffusionUniformKh")


# Native forms of the recovery kernels that the reference's tests write in Python and append to the kernel list.
def DeleteParticle(particles, fieldset):  # tests/common_kernels.py:12-13
    """state >= 50 -> Delete."""
    _device_only("DeleteParticle")


def DeleteOutOfBounds(particles, fieldset):  # tests/test_advection.py:157-161
    """ErrorOutOfBounds / ErrorThroughSurface -> Delete."""
    _device_only("DeleteOutOfBounds")


def DoNothing(particles, fieldset):  # tests/common_kernels.py:8-9
    """Time passes, nothing moves (the kernel of the reference's loop and output tests)."""
    _device_only("DoNothing")


def MoveEast(particles, fieldset):  # tests/common_kernels.py:16-17
    """particles.dx += 0.1"""
    _device_only("MoveEast")


def MoveNorth(particles, fieldset):  # tests/common_kernels.py:20-21
    """particles.dy += 0.1"""
    _device_only("MoveNorth")


def SubmergeParticle(particles, fieldset):  # tests/test_advection.py:163-174
    """ErrorThroughSurface -> resample UV, dz = 0, z = 0, state = Evaluate."""
    _device_only("SubmergeParticle")


def SampleField(field: str, into):
    """The user kernel every Parcels tutorial writes,

        def SampleP(particles, fieldset):
            particles.p = fieldset.P[particles]

    as a device kernel: ``pset.execute([AdvectionRK4, SampleField("P", into="p")], ...)`` samples scalar field ``field`` at every
    particle's (t, z, y, x) in each step of the kernel loop (kernel.py:206-216) and stores it in the particle Variable ``into``
    (float32 or float64, added with ``Particle.add_variable``), with the reference's status-code side effects of a failed
    sample (field.py:307-378).  The vector form ``SampleField("UV", into=("u", "v"))`` / ``SampleField("UVW", into=("u", "v", "w"))``
    is ``particles.u, particles.v = fieldset.UV[particles]`` (tests/test_particleset_execute.py:195-243: the converted velocity
    components of VectorField.__getitem__, field.py:250-304); ``None`` in the tuple discards a component like ``_`` does.
    Returns a kernel token named ``Sample<field>``."""
    if isinstance(into, (tuple, list)):
        into = tuple(into)
        if not all(v is None or isinstance(v, str) for v in into) or all(v is None for v in into):
            raise TypeError("SampleField(vector_field_name, into=(variable_name | None, ...))")
    if not (isinstance(field, str) and isinstance(into, (str, tuple))):
        raise TypeError("SampleField(field_name, into=variable_name)")

    def token(particles, fieldset):
        _device_only(token.__name__)

    token.__name__ = token.__qualname__ = f"Sample{field}"
    token.__doc__ = f"particles.{into} = fieldset.{field}[particles]"
    token._pk_sample = (field, into)
    return token


# ---- CROCO sigma grids (src/parcels/kernels/_sigmagrids.py; csrc/pk_sigma.h) ----------------------------------------------------
def AdvectionRK2_3D_CROCO(particles, fieldset):  # _sigmagrids.py:38-72
    """Second-order Runge-Kutta advection on CROCO sigma layers with the vertical velocity of the 'W' field (sampled linearly); needs the
    fields h, zeta, Cs_w, W and fieldset.add_context("hc", ...)."""
    _device_only("AdvectionRK2_3D_CROCO")


def SampleFieldCroco(field: str, into: str):
    """The reference's SampleOmegaCroco (_sigmagrids.py:28-35) for any scalar field of a CROCO fieldset ("can be adapted to sample any other
    field on a CROCO sigma grid by replacing 'omega'"):

        sigma = convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
        particles.<into> = fieldset.<field>[particles.t, sigma, particles.y, particles.x, particles]

    as a device kernel.  ``into`` is a float32 / float64 particle Variable.  Returns a kernel token named ``Sample<field>Croco``."""
    if not (isinstance(field, str) and isinstance(into, str)):
        raise TypeError("SampleFieldCroco(field_name, into=variable_name)")

    def token(particles, fieldset):
        _device_only(token.__name__)

    token.__name__ = token.__qualname__ = f"Sample{field}Croco"
    token.__doc__ = f"particles.{into} = fieldset.{field}[particles.t, sigma, particles.y, particles.x, particles]"
    token._pk_sample_sigma = (field, into)
    return token


SampleOmegaCroco = SampleFieldCroco("omega", "omega")  # _sigmagrids.py:28-35
SampleOmegaCroco.__name__ = SampleOmegaCroco.__qualname__ = "SampleOmegaCroco"


def convert_z_to_sigma_croco(fieldset, t, z, y, x, particle=None):
    """Local sigma level of the points (t, z, y, x) of a CROCO fieldset (_sigmagrids.py:6-25): NumPy arrays in, sigma out.

    With ``particle=None`` the whole conversion runs on the device (pk_sigma_croco: the two inner samples of h and zeta are detached).
    With a particle view -- inside a Python kernel on the host path -- h and zeta are sampled attached (``Field.eval(..., particles=)``:
    the view's ``state`` / ``ei`` are updated like by any such sample) and the level scan runs on the sampled values, so that

        sigma = convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
        particles.temp = fieldset.T[particles.t, sigma, particles.y, particles.x, particles]

    works on the host path as in the reference.  Written like that in a kernel the translator accepts (parcels_amd/jit.py), the call is
    compiled into the fused sigma loop and this body does not run."""
    import numpy as np

    from .kernel import croco_parameters

    par = croco_parameters(fieldset, who="convert_z_to_sigma_croco")
    t, z, y, x = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v)) for v in (t, z, y, x)))
    if particle is None:
        return fieldset._engine_or_create().sigma_croco(par, t, z, y, x)
    h = fieldset.h.eval(t, np.zeros_like(z), y, x, particles=particle)
    zeta = fieldset.zeta.eval(t, np.zeros_like(z), y, x, particles=particle)
    sigma_levels, cs_w, hc = par["sigma_levels"], par["cs_w"], par["hc"]
    with np.errstate(all="ignore"):
        z0 = hc * sigma_levels[None, :] + (h[:, None] - hc) * cs_w[None, :]
        zvec = z0 + zeta[:, None] * (1.0 + (z0 / h[:, None]))
        zinds = zvec <= z[:, None]
        zi = np.argmin(zinds, axis=1) - 1
        zi = np.where(zinds.all(axis=1), zvec.shape[1] - 2, zi)
        idx = np.arange(zi.shape[0])
        return sigma_levels[zi] + (z - zvec[idx, zi]) * (sigma_levels[zi + 1] - sigma_levels[zi]) / (zvec[idx, zi + 1] - zvec[idx, zi])


# ---- particle-particle interaction (docs/user_guide/examples/tutorial_interaction.ipynb; csrc/pk_interact.hip) -------------------------
def _check_number(who, name, value, positive):
    import math
    import numbers

    import numpy as np

    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f"{who}: {name} must be a {'finite positive' if positive else 'finite'} number, got {type(value).__name__}")
    value = float(value)
    if not math.isfinite(value) or (positive and not value > 0.0):
        raise ValueError(f"{who}: {name} must be a {'finite positive' if positive else 'finite'} number, got {value!r}")
    return value


def _check_interaction_options(who, z, mesh):
    from .fieldset import FieldSet
    from .xgrid import FlatMesh, SphericalMesh

    if not isinstance(z, bool):
        raise TypeError(f"{who}: z must be True or False, got {type(z).__name__}")
    if not isinstance(mesh, (FieldSet, FlatMesh, SphericalMesh)) and not (isinstance(mesh, str) and mesh in ("flat", "spherical")):
        raise ValueError(f"{who}: mesh must be 'flat', 'spherical', a SphericalMesh or a FieldSet. Got {mesh=!r}")


def AttractTowards(sources: str, radius, velocity, *, z=False, mesh="flat", max_pairs=None):
    """The attraction kernel of the interaction tutorial as a built-in kernel: every particle moves with speed ``velocity`` towards each
    source particle closer than ``radius``.  ``sources`` names a particle Variable of any bool or numeric dtype (non-zero = source; it
    stays on the host and no device kernel of the list may write it).  Returns a kernel token named ``AttractTowards_<sources>`` whose
    body is the definition::

        nb = pa.neighbors(particles, radius, z=z, mesh=mesh, max_pairs=max_pairs,
                          sources=np.asarray(particles.<sources>) != 0, include_coincident=False)
        particles.dx += nb.sum(nb.dx / nb.dist) * velocity * particles.dt        # (S * velocity) * dt, left to right
        particles.dy += nb.sum(nb.dy / nb.dist) * velocity * particles.dt
        particles.dz += nb.sum(nb.dz / nb.dist) * velocity * particles.dt        # with z=True

    ``mesh`` takes what ``pa.neighbors`` takes ("flat", "spherical", a SphericalMesh, a FieldSet) and is never guessed.  On a spherical
    mesh the same formula is correct: ``nb.dx`` is in degrees and already wrapped across the antimeridian, ``nb.dist`` is in metres and
    ``velocity`` in m/s, and cos(lat) cancels between the two, so the displacement comes out in degrees.  ``max_pairs`` has the meaning
    and the error of ``pa.neighbors``.

    A kernel list of built-in kernels and these tokens runs on the device-resident particle columns (parcels_amd/interactkernels.py);
    next to a Python function, in RK45 mode, on a UxGrid, next to a CROCO kernel or in a multi-process run the body above runs in the
    host loop like any user kernel."""
    who = "AttractTowards"
    if not isinstance(sources, str):
        raise TypeError(f"{who}: sources must be the name of a particle Variable, got {type(sources).__name__}")
    radius = _check_number(who, "radius", radius, positive=True)
    velocity = _check_number(who, "velocity", velocity, positive=False)
    _check_interaction_options(who, z, mesh)
    if max_pairs is not None:
        import numbers

        if isinstance(max_pairs, bool) or not isinstance(max_pairs, numbers.Integral):
            raise TypeError(f"{who}: max_pairs must be a non-negative integer or None, got {type(max_pairs).__name__}")
        if max_pairs < 0:
            raise ValueError(f"{who}: max_pairs must be a non-negative integer or None, got {max_pairs}")
        max_pairs = int(max_pairs)

    def token(particles, fieldset):
        import numpy as np

        from . import interaction

        nb = interaction.neighbors(particles, radius, z=z, mesh=mesh, max_pairs=max_pairs,
                                   sources=np.asarray(getattr(particles, sources)) != 0, include_coincident=False)
        particles.dx += nb.sum(nb.dx / nb.dist) * velocity * particles.dt
        particles.dy += nb.sum(nb.dy / nb.dist) * velocity * particles.dt
        if z:
            particles.dz += nb.sum(nb.dz / nb.dist) * velocity * particles.dt

    token.__name__ = token.__qualname__ = f"AttractTowards_{sources}"
    token.__doc__ = (f"particles.dx, .dy{', .dz' if z else ''} += sum over the particles.{sources} != 0 within {radius!r} of (d / dist) "
                     f"* {velocity!r} * particles.dt")
    token._pk_interact = {"kind": "attract", "sources": sources, "radius": radius, "velocity": velocity, "z": z, "mesh": mesh, "max_pairs": max_pairs}
    return token


def MergeNearest(mass: str, radius, *, z=False, mesh="flat"):
    """The merge kernel of the interaction tutorial as a built-in kernel: two particles that are each other's nearest neighbour within
    ``radius`` merge -- the heavier keeps the summed mass (equal masses: the lower index keeps), the other is deleted.  ``mass`` names a
    float32 or float64 particle Variable; it becomes a device Variable.  Returns a kernel token named ``MergeNearest_<mass>`` whose body
    is the definition::

        j, _ = pa.nearest_neighbor(particles, radius, z=z, mesh=mesh, include_coincident=False)
        i = np.arange(len(j)); mutual = (j >= 0) & (j[np.where(j >= 0, j, 0)] == i) & (i < j)
        pi, pj = i[mutual], j[mutual]; m = particles.<mass>
        big = np.where(m[pj] > m[pi], pj, pi); small = np.where(m[pj] > m[pi], pi, pj)
        m[big] += m[small]                      # in the Variable's storage dtype
        particles.state[small] = StatusCode.Delete

    ``mesh`` as for ``AttractTowards``; where the list runs: see there."""
    who = "MergeNearest"
    if not isinstance(mass, str):
        raise TypeError(f"{who}: mass must be the name of a particle Variable, got {type(mass).__name__}")
    radius = _check_number(who, "radius", radius, positive=True)
    _check_interaction_options(who, z, mesh)

    def token(particles, fieldset):
        import numpy as np

        from . import interaction
        from .statuscodes import StatusCode

        j, _ = interaction.nearest_neighbor(particles, radius, z=z, mesh=mesh, include_coincident=False)
        i = np.arange(len(j))
        mutual = (j >= 0) & (j[np.where(j >= 0, j, 0)] == i) & (i < j)
        pi, pj = i[mutual], j[mutual]
        m = getattr(particles, mass)
        heavier = m[pj] > m[pi]
        big, small = np.where(heavier, pj, pi), np.where(heavier, pi, pj)
        m[big] += m[small]
        particles.state[small] = int(StatusCode.Delete)

    token.__name__ = token.__qualname__ = f"MergeNearest_{mass}"
    token.__doc__ = f"mutual nearest neighbours within {radius!r} merge: the heavier keeps particles.{mass}, the other is deleted"
    token._pk_interact = {"kind": "merge", "mass": mass, "radius": radius, "z": z, "mesh": mesh}
    return token


def interaction_spec(f):
    """The parameters of an AttractTowards / MergeNearest token, or None."""
    return getattr(f, "_pk_interact", None)


def kernel_id(f):
    """PK_KERNEL_* id of a kernel token, or None for a function this package cannot run."""
    if getattr(f, "_pk_sample_sigma", None) is not None:
        return 12  # PK_KERNEL_SAMPLE_SIGMA_CROCO
    if getattr(f, "_pk_sample", None) is not None:
        return 10  # PK_KERNEL_SAMPLE_FIELD
    return KERNEL_IDS.get(f)


KERNEL_IDS = {
    AdvectionEE: 1,
    AdvectionRK2: 2,
    AdvectionRK2_3D: 3,
    AdvectionRK2_3D_CROCO: 11,
    AdvectionRK4: 4,
    AdvectionRK4_3D: 5,
    AdvectionRK45: 6,
    AdvectionDiffusionM1: 7,
    AdvectionDiffusionEM: 8,
    DiffusionUniformKh: 9,
    DeleteParticle: 20,
    DeleteOutOfBounds: 21,
    SubmergeParticle: 22,
    DoNothing: 23,
    MoveEast: 24,
    MoveNorth: 25,
}
