"""CPU: the factories pa.AttractTowards / pa.MergeNearest, their validation at Kernel construction and the routing decision
(parcels_amd/kernels.py, kernel.py, interactkernels.py).  No device: nothing here launches."""

import os
import re
import types

import numpy as np
import pytest

import parcels_amd as pa
from parcels_amd import _hip, interactkernels, kernels
from parcels_amd.kernel import Kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat_fieldset():
    from case_utils import build_fieldset, load_golden

    case, _, _ = load_golden("agrid_flat_rk4_f64")
    return build_fieldset(case)


def pclass():
    variables = [pa.Variable("attractor", dtype=np.bool_, initial=False), pa.Variable("mass", dtype=np.float64, initial=1.0),
                 pa.Variable("count", dtype=np.int32, initial=0), pa.Variable("p", dtype=np.float32, initial=0.0)]
    return pa.get_default_particle(np.float64).add_variable(variables)


PCLASS = pclass()


def make(kernel_list, fs=None, shard=None):
    pset = types.SimpleNamespace(fieldset=fs or flat_fieldset(), _pclass=PCLASS, _shard=shard)
    return Kernel(kernel_list, pset)


# ---- factories -----------------------------------------------------------------------------------------------------------------------
def test_exports_names_and_docstrings():
    assert pa.AttractTowards is kernels.AttractTowards and pa.MergeNearest is kernels.MergeNearest
    assert {"AttractTowards", "MergeNearest"} <= set(kernels.__all__)
    a = pa.AttractTowards("attractor", 0.12, 0.004)
    m = pa.MergeNearest("mass", 0.03, z=True)
    assert a.__name__ == a.__qualname__ == "AttractTowards_attractor" and m.__name__ == "MergeNearest_mass"
    assert "attractor" in a.__doc__ and "0.12" in a.__doc__ and "0.004" in a.__doc__
    assert "mass" in m.__doc__ and "0.03" in m.__doc__
    assert kernels.interaction_spec(a) == {"kind": "attract", "sources": "attractor", "radius": 0.12, "velocity": 0.004, "z": False, "mesh": "flat",
                                           "max_pairs": None}
    assert kernels.interaction_spec(m) == {"kind": "merge", "mass": "mass", "radius": 0.03, "z": True, "mesh": "flat"}
    assert kernels.interaction_spec(pa.AdvectionRK4) is None and kernels.kernel_id(a) is None
    # the signature Kernel asks of every kernel function, and the spherical note of the issue
    assert list(__import__("inspect").signature(a).parameters) == ["particles", "fieldset"]
    doc = " ".join(pa.AttractTowards.__doc__.split())
    assert "degrees" in doc and "metres" in doc and "cos(lat) cancels" in doc


@pytest.mark.parametrize("call, exc, text", [
    (lambda: pa.AttractTowards(3, 0.1, 1.0), TypeError, "AttractTowards: sources must be the name of a particle Variable, got int"),
    (lambda: pa.AttractTowards("a", "0.1", 1.0), TypeError, "AttractTowards: radius must be a finite positive number, got str"),
    (lambda: pa.AttractTowards("a", True, 1.0), TypeError, "AttractTowards: radius must be a finite positive number, got bool"),
    (lambda: pa.AttractTowards("a", 0.0, 1.0), ValueError, "AttractTowards: radius must be a finite positive number, got 0.0"),
    (lambda: pa.AttractTowards("a", -1.0, 1.0), ValueError, "AttractTowards: radius must be a finite positive number, got -1.0"),
    (lambda: pa.AttractTowards("a", np.inf, 1.0), ValueError, "AttractTowards: radius must be a finite positive number, got inf"),
    (lambda: pa.AttractTowards("a", 0.1, None), TypeError, "AttractTowards: velocity must be a finite number, got NoneType"),
    (lambda: pa.AttractTowards("a", 0.1, np.nan), ValueError, "AttractTowards: velocity must be a finite number, got nan"),
    (lambda: pa.AttractTowards("a", 0.1, 1.0, z=1), TypeError, "AttractTowards: z must be True or False, got int"),
    (lambda: pa.AttractTowards("a", 0.1, 1.0, mesh="round"), ValueError, "AttractTowards: mesh must be 'flat', 'spherical', a SphericalMesh or a FieldSet"),
    (lambda: pa.AttractTowards("a", 0.1, 1.0, max_pairs=1.5), TypeError, "AttractTowards: max_pairs must be a non-negative integer or None, got float"),
    (lambda: pa.AttractTowards("a", 0.1, 1.0, max_pairs=-1), ValueError, "AttractTowards: max_pairs must be a non-negative integer or None, got -1"),
    (lambda: pa.MergeNearest(None, 0.1), TypeError, "MergeNearest: mass must be the name of a particle Variable, got NoneType"),
    (lambda: pa.MergeNearest("m", [0.1]), TypeError, "MergeNearest: radius must be a finite positive number, got list"),
    (lambda: pa.MergeNearest("m", np.nan), ValueError, "MergeNearest: radius must be a finite positive number, got nan"),
    (lambda: pa.MergeNearest("m", 0.1, mesh=None), ValueError, "MergeNearest: mesh must be 'flat', 'spherical', a SphericalMesh or a FieldSet"),
])
def test_factory_argument_errors(call, exc, text):
    with pytest.raises(exc, match=re.escape(text)):
        call()


def test_factories_accept_what_neighbors_accepts():
    from parcels_amd.xgrid import SphericalMesh

    fs = flat_fieldset()
    for mesh in ("flat", "spherical", SphericalMesh(), fs):
        assert kernels.interaction_spec(pa.AttractTowards("attractor", np.float32(10.0), 2, mesh=mesh, max_pairs=np.int64(7)))["max_pairs"] == 7
        assert kernels.interaction_spec(pa.MergeNearest("mass", 3, mesh=mesh))["radius"] == 3.0


# ---- Kernel construction ---------------------------------------------------------------------------------------------------------------
def test_kernel_construction_errors():
    fs = flat_fieldset()
    cases = [
        ([pa.AttractTowards("nope", 0.1, 1.0)], ValueError, "AttractTowards_nope: the ParticleClass has no user Variable 'nope'"),
        ([pa.MergeNearest("nope", 0.1)], ValueError, "MergeNearest_nope: the ParticleClass has no user Variable 'nope'"),
        ([pa.AttractTowards("x", 0.1, 1.0)], ValueError, "AttractTowards_x: the ParticleClass has no user Variable 'x'"),
        ([pa.MergeNearest("dt", 0.1)], ValueError, "MergeNearest_dt: the ParticleClass has no user Variable 'dt'"),
        ([pa.MergeNearest("count", 0.1)], TypeError, "MergeNearest_count: Variable 'count' must be float32 or float64, it is int32"),
        ([pa.MergeNearest("attractor", 0.1)], TypeError, "MergeNearest_attractor: Variable 'attractor' must be float32 or float64, it is bool"),
        ([pa.SampleField("U", into="p"), pa.AttractTowards("p", 0.1, 1.0)], ValueError,
         "AttractTowards_p: Variable 'p' is written by a device kernel of the list"),
        ([pa.AttractTowards("mass", 0.1, 1.0), pa.MergeNearest("mass", 0.1)], ValueError,
         "AttractTowards_mass: Variable 'mass' is written by a device kernel of the list"),
        ([pa.AttractTowards("attractor", 2e7, 1.0, mesh="spherical")], ValueError,
         "AttractTowards_attractor: radius: 20000000.0 is not below a quarter of the circumference"),
        ([pa.MergeNearest("mass", 1.1e7, mesh="spherical")], ValueError, "MergeNearest_mass: radius: 11000000.0 is not below a quarter of the circumference"),
    ]
    import warnings

    for kernel_list, exc, text in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (SampleField("U"): "sampling of velocities should normally be done using UV")
            with pytest.raises(exc, match=re.escape(text)):
                make(kernel_list, fs)


def test_kernel_binds_mass_as_a_device_variable_and_keeps_sources_on_the_host():
    fs = flat_fieldset()
    k = make([pa.AdvectionRK4, pa.AttractTowards("attractor", 0.1, 1.0), pa.MergeNearest("mass", 0.03)], fs)
    assert k.device_variables == ["mass"] and k.host_functions == [] and k.interaction_route == "device"
    assert sorted(k.interactions) == [1, 2] and k.interactions[1]["sphere"] is None
    assert k.funcname == "AdvectionRK4AttractTowards_attractorMergeNearest_mass"
    k = make([pa.AttractTowards("count", 0.1, 1.0)], fs)  # any numeric dtype flags sources
    assert k.device_variables == [] and k.interaction_route == "device"
    k = make([pa.MergeNearest("mass", 5e3, mesh="spherical")], fs)
    assert k.interactions[0]["sphere"] > 6e6
    # PK_MAX_EXTRA holds for the device Variables of the tokens like for SampleField's
    many = [pa.Variable(f"m{j}", dtype=np.float64, initial=1.0) for j in range(_hip.PK_MAX_EXTRA + 1)]
    pset = types.SimpleNamespace(fieldset=fs, _pclass=pa.get_default_particle(np.float64).add_variable(many))
    with pytest.raises(ValueError, match=f"at most {_hip.PK_MAX_EXTRA} particle Variables"):
        Kernel([pa.MergeNearest(f"m{j}", 0.1) for j in range(_hip.PK_MAX_EXTRA + 1)], pset)


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def python_kernel(particles, fieldset):
    particles.dx += 1.0


def test_routing_decision_is_a_pure_function():
    route = interactkernels.interaction_route
    one = dict(rk45_mode=False, on_uxgrid=False, multi_process=False)
    a, m = pa.AttractTowards("attractor", 0.1, 1.0), pa.MergeNearest("mass", 0.03)
    assert route([pa.AdvectionRK4], **one) is None and route([python_kernel], **one) is None  # no token: today's routes
    for covered in ([a], [m], [pa.AdvectionRK4, a, m], [pa.DoNothing, a], [pa.MoveEast, a, pa.MoveNorth, m, pa.DeleteParticle],
                    [pa.AdvectionRK4_3D, pa.SampleField("P", into="p"), a], [pa.AdvectionDiffusionEM, m], [pa.AdvectionEE, a, a]):
        assert route(covered, **one) == "device", [f.__name__ for f in covered]
    for uncovered in ([a, python_kernel], [python_kernel, pa.AdvectionRK4, m], [pa.AdvectionRK2_3D_CROCO, a], [pa.SampleOmegaCroco, m],
                      [pa.SampleFieldCroco("T", "p"), a]):
        assert route(uncovered, **one) == "host", [f.__name__ for f in uncovered]
    for flag in ("rk45_mode", "on_uxgrid", "multi_process"):
        assert route([pa.AdvectionRK4, a], **dict(one, **{flag: True})) == "host", flag


def test_kernel_takes_the_route():
    fs = flat_fieldset()
    a, m = pa.AttractTowards("attractor", 0.1, 1.0), pa.MergeNearest("mass", 0.03)
    k = make([pa.AdvectionRK4, a, python_kernel, m], fs)
    assert k.interaction_route == "host" and k.host_functions == ["AttractTowards_attractor", "python_kernel", "MergeNearest_mass"]
    assert k._jit_tried and k.user_program is None and "host loop" in k.jit_report  # nothing of the list is handed to the translator
    assert k.device_variables == ["mass"]
    k = make([pa.AdvectionRK4, a], fs, shard=(0, 2))
    assert k.interaction_route == "host" and k.host_functions == ["AttractTowards_attractor"]
    assert make([pa.AdvectionRK4, a], fs, shard=(0, 1)).interaction_route == "device"
    assert make([pa.AdvectionRK4, python_kernel], fs).interaction_route is None
    fs45 = flat_fieldset()
    fs45.add_context("RK45_tol", 10.0)
    assert make([pa.AdvectionRK4, a], fs45).interaction_route == "host"
    merged = make([pa.AdvectionRK4], fs).merge(make([a, m], fs))
    assert merged.interaction_route == "device" and sorted(merged.interactions) == [1, 2]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_documented_and_abi_9():
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _hip.PK_ABI_VERSION == 9 and re.search(r"#define\s+PK_ABI_VERSION\s+9\b", header)
    for sym in ("pk_interact_host_order", "pk_interact_sources", "pk_interact_prologue", "pk_interact_attract", "pk_interact_merge",
                "pk_interact_epilogue"):
        assert sym in _hip.ABI_SYMBOLS, sym
        assert re.search(r"^int32_t\s+" + sym + r"\s*\(", header, flags=re.M), f"{sym} is not declared in include/parcels_hip.h"
        assert sym in integration, f"{sym} has no row in INTEGRATION.md"
    block = header[header.index("built-in interaction kernels on the device-resident"):header.index("int32_t pk_measure_copy_bandwidth")]
    assert block.count("kernel.py:") >= 5 and "tutorial_interaction.ipynb" in block  # each export cites what it stands for
