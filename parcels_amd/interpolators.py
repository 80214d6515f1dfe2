"""Interpolator markers (mirrors the class names of src/parcels/interpolators/_xinterpolators.py and _uxinterpolators.py).

The arithmetic lives in the HIP kernels (csrc/pk_device.h: xlinear, cgrid_velocity); these classes select it,
exactly as assigning ``Field.interp_method`` does in the reference (field.py:130-135, 244-248).
"""


class ScalarInterpolator:
    kind = None

    def __repr__(self):  # interpolators/_base.py:10-11
        return f"{self.__class__.__name__}(...)"


class VectorInterpolator:
    kind = None

    def __repr__(self):  # interpolators/_base.py:19-20
        return f"{self.__class__.__name__}(...)"


class XLinear(ScalarInterpolator):  # _xinterpolators.py:112-153
    kind = 0


class XConstantField(ScalarInterpolator):  # _xinterpolators.py:156-166
    kind = 1


class XNearest(ScalarInterpolator):  # _xinterpolators.py:505-553
    kind = 2


class CGrid_Tracer(ScalarInterpolator):  # noqa: N801  _xinterpolators.py:335-383
    kind = 3


class XLinearInvdistLandTracer(ScalarInterpolator):  # _xinterpolators.py:556-613
    kind = 4


class XLinear_Velocity(VectorInterpolator):  # noqa: N801  _xinterpolators.py:169-190
    kind = 0


class CGrid_Velocity(VectorInterpolator):  # noqa: N801  _xinterpolators.py:193-332
    kind = 1


class XFreeslip(VectorInterpolator):  # _xinterpolators.py:480-490 (free-slip boundary condition, a = 1, b = 0)
    kind = 2


class XPartialslip(VectorInterpolator):  # _xinterpolators.py:493-502 (partial slip, a = b = 0.5)
    kind = 3


# unstructured meshes (interpolators/_uxinterpolators.py; csrc/pk_ux.h: ux_interp).  They read time level ti only: no interpolation in time.
class UxConstantFaceConstantZC(ScalarInterpolator):  # face-registered, layer centres (zc): piecewise constant
    kind = 5


class UxConstantFaceLinearZF(ScalarInterpolator):  # face-registered, layer interfaces (zf): linear in the vertical
    kind = 6


class UxLinearNodeConstantZC(ScalarInterpolator):  # node-registered, zc: barycentric laterally, piecewise constant vertically
    kind = 7


class UxLinearNodeLinearZF(ScalarInterpolator):  # node-registered, zf: barycentric laterally, linear vertically
    kind = 8


class Ux_Velocity(VectorInterpolator):  # noqa: N801  _uxinterpolators.py:209-229
    kind = 4


UX_SCALAR_INTERPOLATORS = (UxConstantFaceConstantZC, UxConstantFaceLinearZF, UxLinearNodeConstantZC, UxLinearNodeLinearZF)
