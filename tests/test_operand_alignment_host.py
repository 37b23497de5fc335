"""The C ABI's alignment refusals, no GPU: every blob and workspace that the contract holds to 256 bytes (include/stgcn_hip.h,
"Alignment": LDS-DMA sources and targets of fp64 atomics) and the 8-byte ``save_stats`` are refused with STGCN_ERR_ARG and a
message that names the operand.  The pointers are never touched: the check comes before any plan or launch, so made-up
addresses do."""
import ctypes

import pytest

from stgcn_amd import _capi

ERR_ARG = -1
BASE = 0x7F0000001000          # 4096-byte aligned, never dereferenced

# (entry point, index of the operand among the arguments, its name, bytes off the boundary, the demand)
CASES = [("stgcn_tcn_pack", 2, "Wp", 16, 256), ("stgcn_tcn_forward_packed", 1, "Wp", 16, 256), ("stgcn_tcn_forward", 12, "ws", 4, 256),
         ("stgcn_stem_prepare", 10, "prep", 128, 256), ("stgcn_stem_attention", 6, "ws", 4, 256),
         ("stgcn_stem_tail_prepared", 1, "ws", 16, 256), ("stgcn_stem_tail_prepared", 3, "prep", 64, 256),
         ("stgcn_stem_forward_prepared", 6, "prep", 4, 256), ("stgcn_stem_forward_prepared", 8, "ws", 8, 256),
         ("stgcn_agcn_forward_train", 21, "ws", 8, 256), ("stgcn_agcn_forward_train", 26, "save_stats", 4, 8),
         ("stgcn_agcn_backward_train", 34, "ws", 16, 256), ("stgcn_agcn_backward_train", 17, "save_stats", 4, 8),
         ("stgcn_tcn_forward_train", 9, "ws", 4, 256), ("stgcn_tcn_backward_train", 13, "ws", 4, 256),
         ("stgcn_st_attention_forward", 9, "ws", 4, 256), ("stgcn_st_attention_forward_math", 9, "ws", 4, 256),
         ("stgcn_st_attention_forward_train", 16, "ws", 4, 256), ("stgcn_st_attention_backward", 23, "ws", 4, 256)]


def _args(name, skew_at, skew):
    _, argtypes = _capi.PROTOTYPES[name]
    args = []
    for i, t in enumerate(argtypes):
        if t is ctypes.c_void_p:
            args.append(ctypes.c_void_p(None if i == len(argtypes) - 1 else BASE + 4096 * i + (skew if i == skew_at else 0)))
        elif t is ctypes.c_size_t:
            args.append(ctypes.c_size_t(1 << 40))
        elif t is ctypes.c_float:
            args.append(ctypes.c_float(0.1))
        elif t is ctypes.c_uint:
            args.append(ctypes.c_uint(0))
        else:
            args.append(t(4))
    return args


@pytest.mark.parametrize("name,index,operand,skew,demand", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_a_blob_off_its_boundary_is_refused_by_name(name, index, operand, skew, demand):
    lib = _capi.lib()
    assert _capi.PROTOTYPES[name][1][index] is ctypes.c_void_p and skew % demand
    rc = getattr(lib, name)(*_args(name, index, skew))
    msg = lib.stgcn_last_error().decode()
    assert rc == ERR_ARG, (rc, msg)
    assert f"{operand} must be {demand}-byte aligned" in msg and msg.startswith("stgcn_"), msg


def test_the_abi_number_is_unchanged():
    """The checks refuse calls the contract never covered and change no signature: additive, ABI 11."""
    assert _capi.lib().stgcn_version() == _capi.ABI_VERSION == 11
