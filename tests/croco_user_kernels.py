"""Python kernels a CROCO user writes, shared by tests/test_jit_croco_translation.py (CPU: what the translator makes of them) and
tests/test_gpu_croco_user_kernels.py (GPU: the compiled list against the fixtures and against the host path).  Module-level functions: the
translator reads their source and resolves names through their globals."""

import numpy as np

import parcels_amd
import parcels_amd as pa
from parcels_amd import StatusCode, convert_z_to_sigma_croco


def DeleteParticle(particles, fieldset):  # noqa: N802 -- docs/user_guide/examples/tutorial_croco_3D.ipynb, as written there
    any_error = particles.state >= 50
    particles[any_error].state = StatusCode.Delete


def OmegaRecipe(particles, fieldset):  # noqa: N802 -- SampleOmegaCroco (kernels/_sigmagrids.py:28-35) as the Python function it is there
    sigma = convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
    particles.omega = fieldset.omega[particles.t, sigma, particles.y, particles.x, particles]


def TracerRecipe(particles, fieldset):  # noqa: N802 -- croco_utils.host_recipe("temp", "tracer") written statically
    sigma = pa.convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
    particles.tracer = fieldset.temp[particles.t, sigma, particles.y, particles.x, particles]


def Age(particles, fieldset):  # noqa: N802 -- a float32 Variable counted up in float64 seconds
    particles.age += particles.dt


def DeleteOld(particles, fieldset):  # noqa: N802
    old = particles[particles.age > fieldset.max_age]
    old.state = StatusCode.Delete


def DetachedRecipe(particles, fieldset):  # noqa: N802 -- the conversion WITHOUT the particles: rectilinear grids only
    sigma = parcels_amd.convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, None)
    particles.omega = fieldset.omega[particles.t, sigma, particles.y, particles.x, particles]


def LongSpelling(particles, fieldset):  # noqa: N802
    sigma = parcels_amd.kernels.convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, particles)
    particles.omega = fieldset.omega[particles.t, sigma, particles.y, particles.x, particles]


def SelectedRecipe(particles, fieldset):  # noqa: N802 -- the conversion for a selection of the particles, the result used in arithmetic
    deep = particles[particles.z < -5.0]
    sigma = convert_z_to_sigma_croco(fieldset, deep.t, deep.z, deep.y, deep.x, deep)
    deep.omega = np.abs(sigma) * 2.0


def WrongFirstArgument(particles, fieldset):  # noqa: N802
    sigma = convert_z_to_sigma_croco(particles, particles.t, particles.z, particles.y, particles.x, particles)
    particles.omega = sigma


def WrongArity(particles, fieldset):  # noqa: N802
    sigma = convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y)
    particles.omega = sigma


def WrongParticles(particles, fieldset):  # noqa: N802
    sigma = convert_z_to_sigma_croco(fieldset, particles.t, particles.z, particles.y, particles.x, fieldset)
    particles.omega = sigma


def ScalarDepth(particles, fieldset):  # noqa: N802 -- a literal number as a coordinate stays out
    sigma = convert_z_to_sigma_croco(fieldset, particles.t, -1.0, particles.y, particles.x, particles)
    particles.omega = sigma
