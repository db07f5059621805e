"""include/dvsof_census.h: exported, bound and recorded
(tests/golden/abi_signatures_census.json)."""
import ctypes
import json
import pathlib

from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_census_bwd', 'dvsof_census_fwd', 'dvsof_census_workspace_bytes']


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_the_headers_names_are_exported_bound_and_recorded():
    sig = _abi.CENSUS_FUNCTIONS
    assert _lib.declared_census_symbols() == NAMES == sorted(sig)
    raw, bound = ctypes.CDLL(str(_lib.LIB_PATH)), _lib.lib()
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_census.json').read_text())
    assert set(golden) == set(sig)
    for name, (res, args) in sig.items():
        assert hasattr(raw, name), f'{name} declared in dvsof_census.h, not exported'
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
