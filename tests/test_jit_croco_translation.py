"""CPU: what the translator (parcels_amd/jit.py) makes of the Python kernels of a CROCO kernel list -- the stages of a translated
convert_z_to_sigma_croco call, the sigma variant of the generated module, the refusals -- and a cross-compilation of that module for
gfx950 (a build, not a run)."""

import os
import re
import shutil

import numpy as np
import pytest

import croco_user_kernels as uk
import parcels_amd as pa
from croco_utils import croco_fieldset
from parcels_amd import _hip, jit
from tools import make_croco_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not present")
VARS = {"omega": (0, "f64"), "tracer": (1, "f64"), "age": (2, "f32")}


def _fieldset(name):
    fs = croco_fieldset(mg.load(os.path.join(mg.GOLDEN, name + ".npz")))
    fs.add_context("max_age", 2000.0)
    return fs


def _translate(func, name="croco_host_recipe", spatial=np.float64, fs=None):
    fs = fs if fs is not None else _fieldset(name)
    pclass = pa.get_default_particle(spatial).add_variable([pa.Variable("omega", dtype=np.float64, initial=0), pa.Variable("tracer", dtype=np.float64, initial=0),
                                                            pa.Variable("age", dtype=np.float32, initial=0)])
    field_ids = {n: k for k, n in enumerate(n for n, f in fs.fields.items() if not hasattr(f, "U"))}
    return jit.translate(func, pclass, fs, VARS, field_ids, slot_prefix="k0_"), field_ids


def _requests(src):
    """(field expression, conv) of the request every stage but the last ends with"""
    out = []
    for lines in src.stages:
        for ln in lines:
            m = re.search(r"rq\.fidx = ([\w.]+);", ln)
            if m:
                c = re.search(r"rq\.conv = (\d);", ln)
                out.append((m.group(1), int(c.group(1)) if c else 0))
    return out


def test_the_sigma_variant_is_apart_from_every_other():
    header = open(os.path.join(ROOT, "include", "parcels_hip.h")).read()
    assert int(re.search(r"#define\s+PK_USER_SIGMA\s+(\d+)", header).group(1)) == jit.PK_USER_SIGMA == _hip.PK_USER_SIGMA == 2 * _hip.PK_USER_UX
    assert int(re.search(r"#define\s+PK_USER_KEY_SIGMA\s+(\d+)", header).group(1)) == jit.PK_USER_KEY_SIGMA == _hip.PK_USER_KEY_SIGMA
    keys = range(jit.PK_USER_KEY_SIGMA, jit.PK_USER_KEY_SIGMA + 8)
    assert not set(keys) & (set(range(12)) | {jit.PK_USER_KEY_UX})
    src, _ = _translate(uk.DeleteParticle)
    assert not src.sigma and src.sampled == []
    digests = set()
    for key in keys:
        v = key - jit.PK_USER_KEY_SIGMA
        p = jit.UserProgram([src], key, 33 * 16, fast=1)
        assert p.sigma and not p.ux and p.flags == jit.PK_USER_SIGMA  # never PK_USER_RIDE
        assert '#include "pk_sigma.h"' in p.source and "#define PK_SIGMA_KERNELS 1" in p.source and "#define PK_USER_KERNELS 1" in p.source
        assert f"advect_sigma_kernel<{'float' if v & 4 else 'double'}, {(v >> 1) & 1}, {v & 1}>" in p.source and "(size_t)lds_bytes" in p.source
        assert f"key != {key} " in p.source and "abort();" in p.source and "advect_kernel<" not in p.source
        assert p.digest == jit.UserProgram([src], key, 9 * 16).digest  # (the number of levels is the launch's, not the module's)
        digests.add(p.digest)
    assert len(digests) == 8
    for key in (jit.PK_USER_KEY_SIGMA - 1, jit.PK_USER_KEY_SIGMA + 8):
        with pytest.raises(jit.NotTranslatable):
            jit.UserProgram([src], key, 0)


@pytest.mark.parametrize("func", [uk.OmegaRecipe, uk.LongSpelling, uk.TracerRecipe, uk.DetachedRecipe])
def test_the_conversion_is_two_marked_samples_before_the_sample_that_uses_sigma(func):
    """bare name, `pa.`, `parcels_amd.`, `parcels_amd.kernels.`: h, then zeta, both at z = 0 and marked as a conversion; then the field"""
    src, fid = _translate(func)
    field = "temp" if func is uk.TracerRecipe else "omega"
    assert src.sigma and src.sampled == [fid["h"], fid["zeta"], fid[field]]
    assert len(src.stages) == 4 and src.counter is None
    assert _requests(src) == [("a.sigma.fh", 1), ("a.sigma.fzeta", 2), (str(fid[field]), 0)]
    for k in (0, 1):
        (rq,) = [ln for ln in src.stages[k] if "rq.conv" in ln]
        assert "rq.z = 0.0;" in rq and "rq.kind = RQ_SCALAR;" in rq and "rq.f32 = false; rq.zf32 = false;" in rq and "rq.cz = (double)(p.z);" in rq
    use = [ln for ln in src.stages[2] if "rq.fidx" in ln][0]
    sigma = re.search(r"(L\.ul\.k0_s\d+) = L\.r\[3\];", "\n".join(src.stages[2])).group(1)  # where the loop leaves the level
    local = re.search(r"(L\.ul\.k0_l\d+) = " + re.escape(sigma) + ";", "\n".join(src.stages[2])).group(1)  # `sigma = ...`: a local array
    assert f"rq.z = (double)({local});" in use
    assert src.detached == (func is uk.DetachedRecipe)
    if src.detached:  # state and ei restored behind the second sample
        assert "c.state" in src.stages[0][0] and "c.ei0 =" in src.stages[2][0]
    prog = jit.UserProgram([src], jit.PK_USER_KEY_SIGMA + 1, 33 * 16)
    assert prog.sigma and prog.flags == jit.PK_USER_SIGMA and "rq.conv = 2;" in prog.source
    with pytest.raises(jit.NotTranslatable, match="sigma loop"):  # no other loop serves the conversion
        jit.UserProgram([src], 1, 1)


def test_float32_particle_columns_set_the_request_flags():
    src, _ = _translate(uk.OmegaRecipe, spatial=np.float32)
    (rq,) = [ln for ln in src.stages[0] if "rq.conv" in ln]
    assert "rq.f32 = true; rq.zf32 = true;" in rq


def test_the_conversion_for_a_selection_is_a_conditional_request():
    src, fid = _translate(uk.SelectedRecipe)
    assert src.sigma and src.counter is not None and src.sampled == [fid["h"], fid["zeta"]]
    for k in (0, 1):
        (rq,) = [ln for ln in src.stages[k] if "rq.conv" in ln]
        assert re.search(r"if \(L\.ul\.k0_l\d+\) \{ rq\.kind = RQ_SCALAR;", rq)


def test_what_is_not_translated_says_so():
    for func, msg in ((uk.WrongFirstArgument, "convert_z_to_sigma_croco: the first argument"), (uk.WrongArity, "convert_z_to_sigma_croco.*4 arguments"),
                      (uk.WrongParticles, "convert_z_to_sigma_croco: the last argument"), (uk.ScalarDepth, "convert_z_to_sigma_croco: z is not a numeric array")):
        with pytest.raises(jit.NotTranslatable, match=msg):
            _translate(func)
    with pytest.raises(jit.NotTranslatable, match="without particles on a curvilinear grid"):
        _translate(uk.DetachedRecipe, "croco_curv_flat_f64data_f64part")
    assert _translate(uk.OmegaRecipe, "croco_curv_flat_f64data_f64part")[0].sigma  # the attached form is translated there
    # croco_parameters is checked at translation: its error is the reason
    fs = _fieldset("croco_host_recipe")
    del fs.context["hc"]
    with pytest.raises(jit.NotTranslatable, match=r"OmegaRecipe needs fieldset.add_context\('hc'"):
        _translate(uk.OmegaRecipe, fs=fs)
    # the function the test suite builds with getattr / setattr stays on the host path
    from croco_utils import host_recipe

    with pytest.raises(jit.NotTranslatable):
        _translate(host_recipe("temp", "tracer"))


@needs_hipcc
def test_the_sigma_module_cross_compiles_for_gfx950(tmp_path, monkeypatch):
    """the tutorial's DeleteParticle and the static recipe in one module of the C-grid, float64, rectilinear variant"""
    monkeypatch.setenv("PARCELS_AMD_JIT_CACHE", str(tmp_path))
    a, _ = _translate(uk.DeleteParticle)
    b, _ = _translate(uk.OmegaRecipe)
    b.decl = [d.replace("k0_", "k1_") for d in b.decl]
    b.stages = [[ln.replace("k0_", "k1_") for ln in st] for st in b.stages]
    prog = jit.UserProgram([a, b], jit.PK_USER_KEY_SIGMA + 1, 33 * 16)
    path = prog.build()
    assert os.path.dirname(path) == str(tmp_path) and os.path.getsize(path) > 0
    blob = open(path, "rb").read()
    assert b"pk_user_launch" in blob and b"advect_sigma_kernel" in blob and b"sigma_points_kernel" not in blob
