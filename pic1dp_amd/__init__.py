"""pic1dp_amd -- MI355X-native time-step engine for 1-D electrostatic delta-f PIC
with the behaviour of the hot path of wenjundeng/pic1dp (PIC1D-PETSc).

The product is libpic1dp_hip.so (hand-written gfx950 HIP kernels behind the C
ABI of include/pic1dp_hip.h).  This package is the thin Python host mirroring the
reference's procedure names.  Importing it loads the library; if the library is
missing the import fails -- there is no CPU fallback.
"""
from . import _lib

_lib.load()  # fail loudly, now, if the HIP library is absent

from ._lib import Input, Layout, Pic1dpError, Hermite, Select, Zoom  # noqa: E402,F401
from .engine import Pic1dp, charge_quantum, checkpoint_info, checkpoint_verify, host_digest, host_select, load_origin, load_uniforms, device_count, diag_convert, diag_quanta, diag_quantise, field_transform_supported, make_input, moments_convert, moments_limbs_len, moments_quanta, power_convert, power_limbs_len, power_quantum, select_thin, tuning_build, host_zoom, make_zoom, zoom_convert, zoom_len, make_hermite, hermite_len, host_hermite, hermite_tables, hermite_functions, hermite_series  # noqa: E402,F401
from . import parallel  # noqa: E402,F401

__all__ = ["Pic1dp", "make_input", "checkpoint_info", "checkpoint_verify", "host_digest", "host_select", "select_thin", "host_zoom", "zoom_convert", "zoom_len", "make_zoom", "Zoom", "make_hermite", "hermite_len", "host_hermite", "hermite_tables", "hermite_functions", "hermite_series", "Hermite", "load_origin", "load_uniforms", "charge_quantum", "diag_quanta", "diag_quantise", "diag_convert", "moments_quanta", "moments_limbs_len", "moments_convert", "power_quantum", "power_limbs_len", "power_convert", "device_count", "field_transform_supported", "tuning_build", "Input", "Layout", "Select", "Pic1dpError", "parallel"]
