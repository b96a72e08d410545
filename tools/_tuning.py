"""Knobs of the tuning build (disn_amd/csrc/tuning.hpp).  Tools only: build it with
`python -m disn_amd.csrc.build --tuning` and run the tool with
DISN_AMD_LIB=disn_amd/csrc/libdisn_amd_tuning.so (the product library has no knobs)."""
import ctypes as C

KEYS = {"fused_safe": 0, "aux_cu_mode": 1}


def set_knob(name: str, value: int) -> None:
    from disn_amd import _lib
    h = _lib.lib()
    try:
        fn = h.disn_tuning_set
    except AttributeError:
        raise SystemExit("this tool needs the tuning build: python -m disn_amd.csrc.build --tuning and "
                         "DISN_AMD_LIB=disn_amd/csrc/libdisn_amd_tuning.so")
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int]
    if fn(KEYS[name], int(value)) != 0:
        raise ValueError(name)
