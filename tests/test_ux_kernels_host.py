"""CPU: the kernel list on an unstructured mesh (UxGrid) -- validation of the diffusion kernels, the fixtures of
tools/make_ux_kernels_golden.py against the live reference, and the user-kernel module of the UxGrid program (parcels_amd/jit.py):
translation, its variant key, and a cross-compilation for gfx950."""

import glob
import os
import re
import shutil

import numpy as np
import pytest

import parcels_amd as pa
from oracle import ref_shim
from parcels_amd import StatusCode, _hip, jit
from parcels_amd.kernel import Kernel
from tools import make_ux_kernels_golden as gk
from ux_kernels_utils import uxk_fieldset, uxk_pset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gk.GOLDEN, "uxk_*.npz")))
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference sources not present")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not present")


def _case(name):
    return gk.load(os.path.join(gk.GOLDEN, name + ".npz"))


def test_fixtures_cover_the_cases_and_are_small():
    assert FIXTURES == sorted(gk.cases())
    assert len(FIXTURES) == 10
    counts = set()
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(gk.GOLDEN, n + ".npz")) < 64 << 10, n
        case = _case(n)
        counts.add(len(case["x"]))
        assert case["faces"].shape[0] == 200 and 8 <= abs(case["runtime"] / case["dt"]) <= 12
        assert case["conditions"]["kh_min"] >= 0 and case["conditions"].get("gradient_fraction", 1.0) >= 0.5
        if case["mesh"] == "spherical":
            assert case["spatial_dtype"] == "float64" and case["conditions"]["rounded_trig_max_dev"] <= 1e-12 * 50.0
            assert all(d[2] == "n_face" for _, d in case["fields"].values())
    assert counts == {1, 63, 64, 65, 257}
    edge = _case("uxk_flat_face_m1_edge")
    assert edge["err"] == "GridSearchingError" and np.any(edge["ref"]["state"] == StatusCode.ErrorGridSearching)


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_diffusion_kernels_are_accepted_on_a_uxgrid():
    fs = uxk_fieldset(_case("uxk_flat_face_em"))
    assert isinstance(fs.Kh_zonal.grid, pa.UxGrid)
    pset = uxk_pset(_case("uxk_flat_face_em"), fs)
    for k in (pa.AdvectionDiffusionM1, pa.AdvectionDiffusionEM, pa.DiffusionUniformKh):
        kern = Kernel([k], pset)
        assert kern.kernel_ids == [pa.kernels.kernel_id(k)] and not kern.host_functions
    fs = uxk_fieldset(_case("uxk_sph_rk4_uniformkh_const"))  # Kh from add_constant_field: its own (spherical) one-point grid next to the mesh
    assert not isinstance(fs.Kh_zonal.grid, pa.UxGrid) and fs.Kh_zonal.grid._mesh.is_spherical()
    Kernel([pa.AdvectionRK4, pa.DiffusionUniformKh], uxk_pset(_case("uxk_sph_rk4_uniformkh_const"), fs))


def test_diffusion_kernels_need_kh_and_dres_on_a_uxgrid():
    case = _case("uxk_flat_face_em")
    no_kh = dict(case, fields={k: v for k, v in case["fields"].items() if k in ("U", "V")})
    fs = uxk_fieldset(no_kh)
    for k in (pa.AdvectionDiffusionM1, pa.AdvectionDiffusionEM, pa.DiffusionUniformKh):
        with pytest.raises(ValueError, match=f"{k.__name__} needs the field Kh_zonal"):
            Kernel([k], uxk_pset(no_kh, fs))
    only_zonal = dict(case, fields={k: v for k, v in case["fields"].items() if k != "Kh_meridional"})
    with pytest.raises(ValueError, match="needs the field Kh_meridional"):
        Kernel([pa.DiffusionUniformKh], uxk_pset(only_zonal, uxk_fieldset(only_zonal)))
    no_dres = dict(case, context={})
    fs = uxk_fieldset(no_dres)
    for k in (pa.AdvectionDiffusionM1, pa.AdvectionDiffusionEM):
        with pytest.raises(ValueError, match=r"needs fieldset.add_context\('dres', ...\)"):
            Kernel([k], uxk_pset(no_dres, fs))
    Kernel([pa.DiffusionUniformKh], uxk_pset(no_dres, fs))  # (no gradient term: no dres)


@needs_reference
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_regenerates_from_the_reference(name):
    """tools/make_ux_kernels_golden.py run on the live reference gives the committed arrays (and holds the generator's conditions)"""
    arrs = gk.generate(name, gk.cases()[name])
    with np.load(os.path.join(gk.GOLDEN, name + ".npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(arrs)
        for k in z.files:
            assert np.array_equal(z[k], arrs[k], equal_nan=z[k].dtype.kind == "f"), (name, k)


# ---- the user module of the UxGrid program ---------------------------------------------------------------------------------------------
def Age(particles, fieldset):  # noqa: N802
    particles.age += particles.dt
    particles.state = np.where(particles.age > fieldset.max_age, StatusCode.Delete, particles.state)


def SampleT(particles, fieldset):  # noqa: N802
    particles.temp = fieldset.Kh_zonal[particles]
    u, v = fieldset.UV[particles.t, particles.z, particles.y, particles.x - 0.1, particles]
    particles.dx += u * particles.dt


def DetachedT(particles, fieldset):  # noqa: N802
    particles.temp = fieldset.Kh_zonal[particles.t, particles.z, particles.y, particles.x]


def DetachedUV(particles, fieldset):  # noqa: N802
    u, v = fieldset.UV[particles.t, particles.z, particles.y, particles.x]
    particles.dx += u * particles.dt


def SampleU(particles, fieldset):  # noqa: N802
    particles.temp = fieldset.U[particles]


def _translate(func, name="uxk_flat_face_em"):
    case = _case(name)
    fs = uxk_fieldset(case)
    fs.add_context("max_age", 50.0)
    pclass = pa.get_default_particle(np.float64).add_variable([pa.Variable("age", dtype=np.float32, initial=0), pa.Variable("temp", dtype=np.float64, initial=0)])
    field_ids = {n: k for k, n in enumerate(n for n, f in fs.fields.items() if not hasattr(f, "U"))}
    return jit.translate(func, pclass, fs, {"age": (0, "f32"), "temp": (1, "f64")}, field_ids, slot_prefix="k0_")


def test_variant_key_of_the_uxgrid_module_is_no_structured_key():
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    assert int(re.search(r"#define\s+PK_USER_KEY_UX\s+(\d+)", header).group(1)) == jit.PK_USER_KEY_UX == _hip.PK_USER_KEY_UX
    assert int(re.search(r"#define\s+PK_USER_UX\s+(\d+)", header).group(1)) == jit.PK_USER_UX == _hip.PK_USER_UX
    structured = range(12)  # (float32 fields ? 6 : 0) + (curvilinear ? 3 : 0) + min(interp_uv, 2)
    assert jit.PK_USER_KEY_UX not in structured
    assert jit.PK_USER_UX not in (_hip.PK_USER_RIDE, _hip.PK_USER_SAMPLES_UV, _hip.PK_USER_SAMPLES_UVW)
    src = _translate(Age)
    ux = jit.UserProgram([src], jit.PK_USER_KEY_UX, 0)
    assert ux.ux and ux.flags & jit.PK_USER_UX and not ux.flags & _hip.PK_USER_RIDE
    assert "advect_ux_kernel<0>" in ux.source and "#define PK_UX_KERNELS" in ux.source and '#include "pk_ux.h"' in ux.source
    assert f"key != {jit.PK_USER_KEY_UX}" in ux.source and "advect_kernel<" not in ux.source
    assert "advect_ux_kernel<1>" in jit.UserProgram([src], jit.PK_USER_KEY_UX, 0, particles_f32=True).source
    digests = {ux.digest}
    for key in structured:
        for fast in (0, 1):
            p = jit.UserProgram([src], key, 1, fast=fast)
            assert not p.ux and not p.flags & jit.PK_USER_UX and "advect_ux_kernel" not in p.source and f"key != {key} " in p.source
            digests.add(p.digest)
    assert len(digests) == 1 + 2 * len(structured)
    with pytest.raises(jit.NotTranslatable):
        jit.UserProgram([src], jit.PK_USER_KEY_UX, 1)  # the UxGrid program stages nothing in LDS
    with pytest.raises(jit.NotTranslatable):
        jit.UserProgram([src], 13, 0)


@needs_hipcc
@pytest.mark.parametrize("func", [Age, SampleT])
def test_uxgrid_user_module_cross_compiles_for_gfx950(func, tmp_path, monkeypatch):
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", str(tmp_path))
    src = _translate(func)
    assert src.sampled == [] if func is Age else (isinstance(src.sampled[0], int) and src.sampled[1:] == ["UV"])
    prog = jit.UserProgram([src], jit.PK_USER_KEY_UX, 0)
    assert prog.sample_flags == (0 if func is Age else _hip.PK_USER_SAMPLES_UV)
    path = prog.build()
    assert os.path.dirname(path) == str(tmp_path) and os.path.getsize(path) > 0
    blob = open(path, "rb").read()
    assert b"pk_user_launch" in blob and b"advect_ux_kernel" in blob


def test_sample_without_particles_is_not_translatable_on_a_uxgrid():
    for f in (DetachedT, DetachedUV):
        with pytest.raises(jit.NotTranslatable, match="UxGrid"):
            _translate(f)
    with pytest.raises(jit.NotTranslatable, match="UxGrid"):  # also for a constant field next to the mesh
        _translate(DetachedT, "uxk_flat_rk4_uniformkh_const")
    with pytest.raises(jit.NotTranslatable, match="velocity component by itself"):  # as on structured grids
        _translate(SampleU)
    assert len(_translate(SampleT).stages) == 3  # the attached forms are stages like anywhere else


def test_only_rk45_and_submerge_stay_refused_on_a_uxgrid():
    from parcels_amd import kernel as kmod

    assert kmod._NOT_ON_UXGRID == (pa.AdvectionRK45, pa.SubmergeParticle)
