"""User kernels that sample NAMED vector fields -- wind, Stokes drift, an unbeaching displacement -- written for this project's tests of
`fieldset.<Name>[...]` in the fused step loop.  One module, imported by the fixture generator (tools/make_named_vector_golden.py, which runs
them through the reference's own kernel loop) and by the tests (tests/test_named_vectors_host.py, tests/test_gpu_named_vectors.py, which run
them compiled and on the host path); module level, because the translator reads a kernel's source."""
import numpy as np

from parcels_amd import StatusCode


def WindMidpoint(particles, fieldset):
    """Windage with a midpoint step: a fraction `fieldset.windage` of the wind at the half-step position moves the particle."""
    uw, vw = fieldset.Wind[particles]
    half = 0.5 * particles.dt
    ym = particles.y + vw * fieldset.windage * half
    xm = particles.x + uw * fieldset.windage * half
    uw, vw = fieldset.Wind[particles.t + half, particles.z, ym, xm, particles]
    particles.dx += uw * fieldset.windage * particles.dt
    particles.dy += vw * fieldset.windage * particles.dt


def StokesEuler(particles, fieldset):
    """Stokes drift, forward Euler, from a vector field of another dataset (`fs_currents + fs_stokes`)."""
    us, vs = fieldset.UVstokes[particles]
    particles.dx += us * particles.dt
    particles.dy += vs * particles.dt


def SampleThree(particles, fieldset):
    """A three-component vector field sampled into three Variables."""
    particles.u2, particles.v2, particles.w2 = fieldset.UVW2[particles]


def Unbeach(particles, fieldset):
    """Particles that drifted into the shallow band (`fieldset.shore`, in units of x) are pushed back by a displacement field sampled a
    little seaward of them; the others sample nothing."""
    ashore = particles[particles.x < fieldset.shore]
    du, dv = fieldset.Disp[ashore.t, ashore.z, ashore.y, ashore.x - 0.1, ashore]
    ashore.dx += du * ashore.dt
    ashore.dy += dv * ashore.dt
    ashore.beached += 1


def WindDetached(particles, fieldset):
    """The wind at the particles' positions taken WITHOUT the particles: no state change, no `ei` update (rectilinear grids)."""
    uw, vw = fieldset.Wind[particles.t, particles.z, particles.y, particles.x]
    particles.dx += uw * fieldset.windage * particles.dt
    particles.dy += vw * fieldset.windage * particles.dt


def NoSample(particles, fieldset):
    """Samples nothing: what a list with a detached sample is compared with."""
    particles.dx += 0.0


def DeleteParticle(particles, fieldset):
    """Delete every particle that carries an error code."""
    particles[particles.state >= 50].state = StatusCode.Delete
