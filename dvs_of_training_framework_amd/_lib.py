"""ctypes binding of libdvsof_hip.so (C ABI: include/dvsof.h).

Signatures, struct layouts and constants are not written down here: _abi.py
reads them from the header when the package is imported.  To add an entry
point, declare it in include/dvsof.h and update
tests/golden/abi_signatures.json, the recorded table a review sees change;
or, leaving that table as it is, in an extension header (_abi.EXTENSION_PATHS:
include/dvsof_contrast.h, recorded in tests/golden/abi_signatures_contrast.json;
_abi.CONTRAST_MULTI_PATH: include/dvsof_contrast_multi.h, recorded in
tests/golden/abi_signatures_contrast_multi.json; _abi.IWE_MULTI_PATH:
include/dvsof_iwe_multi.h, recorded in tests/golden/abi_signatures_iwe_multi.json;
_abi.LOSS_FRAMELESS_PATH: include/dvsof_loss_frameless.h, recorded in
tests/golden/abi_signatures_loss_frameless.json; _abi.CONTRAST_PYRAMID_PATH:
include/dvsof_contrast_pyramid.h, recorded in
tests/golden/abi_signatures_contrast_pyramid.json; _abi.AVG_TIMESTAMP_PATH:
include/dvsof_avg_timestamp.h, recorded in
tests/golden/abi_signatures_avg_timestamp.json; _abi.AVG_TIMESTAMP_PYRAMID_PATH:
include/dvsof_avg_timestamp_pyramid.h, recorded in
tests/golden/abi_signatures_avg_timestamp_pyramid.json;
_abi.EVENT_TERMS_ENCODED_PATH: include/dvsof_event_terms_encoded.h, recorded in
tests/golden/abi_signatures_event_terms_encoded.json;
_abi.IWE_AVG_TIMESTAMP_PATH: include/dvsof_iwe_avg_timestamp.h, recorded in
tests/golden/abi_signatures_iwe_avg_timestamp.json).

There is NO fallback: if the library is missing or a call fails the product
raises.  PyTorch is used only for device memory and streams; every entry
point gets raw device pointers and the current HIP stream.
"""
import ctypes
import re

import torch

from . import _abi
from ._switches import library_path

LIB_PATH = library_path()       # the product build unless DVSOF_LIB_PATH / DVSOF_PROBE_LIB say otherwise
HEADER_PATH = _abi.HEADER_PATH
CONSTANTS = _abi.CONSTANTS     # {name: int}: every #define DVSOF_* and enum member of the header
STRUCTS = _abi.STRUCTS         # {typedef name: ctypes.Structure}
MAX_SCALES = CONSTANTS['DVSOF_MAX_SCALES']
LossScale = STRUCTS['dvsof_loss_scale_t']

# {name: (restype, argtypes)} of every entry point, derived from the header
_SIGNATURES = _abi.FUNCTIONS
# the same of the extension headers (include/dvsof_contrast.h)
_EXTENSION_SIGNATURES = _abi.EXTENSION_FUNCTIONS
# and of include/dvsof_contrast_multi.h, a table of its own
_CONTRAST_MULTI_SIGNATURES = _abi.CONTRAST_MULTI_FUNCTIONS
# and of include/dvsof_iwe_multi.h, likewise
_IWE_MULTI_SIGNATURES = _abi.IWE_MULTI_FUNCTIONS
# and of include/dvsof_loss_frameless.h, likewise
_LOSS_FRAMELESS_SIGNATURES = _abi.LOSS_FRAMELESS_FUNCTIONS
# and of include/dvsof_contrast_pyramid.h, with the level table it passes by value
_CONTRAST_PYRAMID_SIGNATURES = _abi.CONTRAST_PYRAMID_FUNCTIONS
ContrastLevel = _abi.CONTRAST_PYRAMID_STRUCTS['dvsof_contrast_level_t']
ContrastLevels = _abi.CONTRAST_PYRAMID_STRUCTS['dvsof_contrast_levels_t']
# and of include/dvsof_avg_timestamp.h, functions only
_AVG_TIMESTAMP_SIGNATURES = _abi.AVG_TIMESTAMP_FUNCTIONS
# and of include/dvsof_avg_timestamp_pyramid.h, which takes the level table above
_AVG_TIMESTAMP_PYRAMID_SIGNATURES = _abi.AVG_TIMESTAMP_PYRAMID_FUNCTIONS
# and of include/dvsof_event_terms_encoded.h, the two terms on the encoded event columns
_EVENT_TERMS_ENCODED_SIGNATURES = _abi.EVENT_TERMS_ENCODED_FUNCTIONS
# and of include/dvsof_iwe_avg_timestamp.h, the average-timestamp images of the validation metric
_IWE_AVG_TIMESTAMP_SIGNATURES = _abi.IWE_AVG_TIMESTAMP_FUNCTIONS

_lib = None
LOADED_STAT = None


def declared_symbols():
    """Names of all entry points include/dvsof.h declares."""
    text = HEADER_PATH.read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(dvsof_[a-z0-9_]+)\s*\(', text)))


def _declared_in(paths):
    found = set()
    for path in paths:
        text = re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)
        found |= set(re.findall(r'\b(dvsof_[a-z0-9_]+)\s*\(', text))
    return sorted(found)


def declared_extension_symbols():
    """Names of all entry points the extension headers declare."""
    return _declared_in(_abi.EXTENSION_PATHS)


def declared_contrast_multi_symbols():
    """Names of all entry points include/dvsof_contrast_multi.h declares."""
    return _declared_in((_abi.CONTRAST_MULTI_PATH,))


def declared_iwe_multi_symbols():
    """Names of all entry points include/dvsof_iwe_multi.h declares."""
    return _declared_in((_abi.IWE_MULTI_PATH,))


def declared_loss_frameless_symbols():
    """Names of all entry points include/dvsof_loss_frameless.h declares."""
    return _declared_in((_abi.LOSS_FRAMELESS_PATH,))


def declared_contrast_pyramid_symbols():
    """Names of all entry points include/dvsof_contrast_pyramid.h declares."""
    return _declared_in((_abi.CONTRAST_PYRAMID_PATH,))


def declared_avg_timestamp_symbols():
    """Names of all entry points include/dvsof_avg_timestamp.h declares."""
    return _declared_in((_abi.AVG_TIMESTAMP_PATH,))


def declared_avg_timestamp_pyramid_symbols():
    """Names of all entry points include/dvsof_avg_timestamp_pyramid.h declares."""
    return _declared_in((_abi.AVG_TIMESTAMP_PYRAMID_PATH,))


def declared_event_terms_encoded_symbols():
    """Names of all entry points include/dvsof_event_terms_encoded.h declares."""
    return _declared_in((_abi.EVENT_TERMS_ENCODED_PATH,))


def declared_iwe_avg_timestamp_symbols():
    """Names of all entry points include/dvsof_iwe_avg_timestamp.h declares."""
    return _declared_in((_abi.IWE_AVG_TIMESTAMP_PATH,))


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C dvs_of_training_framework_amd/csrc`. '
                'There is no CPU fallback for the HIP hot path.')
        _lib = ctypes.CDLL(str(LIB_PATH))
        st = LIB_PATH.stat()
        global LOADED_STAT      # the file these code objects came from (_audit.py)
        LOADED_STAT = (st.st_ino, st.st_size, st.st_mtime_ns)
        for name, (res, args) in {**_SIGNATURES, **_EXTENSION_SIGNATURES, **_CONTRAST_MULTI_SIGNATURES,
                                  **_IWE_MULTI_SIGNATURES, **_LOSS_FRAMELESS_SIGNATURES,
                                  **_CONTRAST_PYRAMID_SIGNATURES, **_AVG_TIMESTAMP_SIGNATURES,
                                  **_AVG_TIMESTAMP_PYRAMID_SIGNATURES,
                                  **_EVENT_TERMS_ENCODED_SIGNATURES,
                                  **_IWE_AVG_TIMESTAMP_SIGNATURES}.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = res, args
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().dvsof_error_string(rc).decode()
        raise RuntimeError(f'{what} failed: {msg} (code {rc})')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream():
    """Current torch HIP stream as a raw hipStream_t (one C call: this runs
    before every kernel launch, ~120 times per training step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                'the dvsof HIP path needs device tensors (got a CPU tensor); '
                'there is no CPU implementation in this package')
