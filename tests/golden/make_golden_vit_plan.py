"""Records what the host code of the heads' transformer block decides, for tests/test_vit_plan_host.py to ask again:
tests/golden/vit_plan_parent.json.  Run it on the commit BEFORE the block's plan (csrc/vit.h ``plan_block``) existed - the
fixture pins that moving the decisions into one place changed none of them; needs no GPU.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_golden_vit_plan.py [--out file.json]

Three sections:
  queries : the coverage queries tests/golden/vit_queries_abi11.json does not hold, over that maker's grids
  status  : the status codes of the four entry points that read the plan, over every flag word x five shapes x (all pointers
            NULL | distinct dummy host addresses with zero-byte buffers).  With zero bytes a call that passes every check ends
            in STGCN_ERR_WORKSPACE, so none reaches a launch.  Per case the status and which tokens the message holds.
  flags   : the flag word a ``Block`` hands to ``F.vit_block_forward`` and ``_BlockTrain.apply``, over its modes, the two
            environment defaults, ``small_tiles`` and a resident and a streaming length
"""
import argparse
import ctypes
import importlib.util
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

_spec = importlib.util.spec_from_file_location("make_golden_vit_queries", os.path.join(HERE, "make_golden_vit_queries.py"))
mq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mq)

QKV_F32, TILE_AUTO, TILE_64, BF16, TRAIN_BF16 = 0x2000, 0x10000, 0x20000, 0x40000, 0x200000
FLAGS = [low | q | t | b | tb for low, q, t, b, tb in
         itertools.product((0, 1, 2, 3), (0, QKV_F32), (0, TILE_AUTO, TILE_64), (0, BF16), (0, TRAIN_BF16))]
SHAPES = ((2, 22, 256, 8, 512), (2, 300, 256, 8, 512), (2, 4097, 256, 8, 512), (2, 22, 384, 8, 512), (0, 22, 256, 8, 512))
LINEAR_SHAPE = (44, 256, 100)
ENTRIES = ("stgcn_vit_block_forward", "stgcn_vit_block_forward_train", "stgcn_vit_block_backward", "stgcn_vit_linear_backward")
TOKENS = ("STGCN_VIT_BF16", "STGCN_VIT_TILE", "STGCN_VIT_TRAIN_BF16", "null", "math", "workspace", "saved buffer")

MATH_MODES = (None, "f32", "bf16x3", "mixed", "bf16", "mixed|TILE_64", "bf16|TILE_AUTO")
TRAIN_MODES = (None, "f32", "bf16x3", "mixed", "bf16")
ENV_MATH = (None, "f32", "bf16")
ENV_TRAIN_MATH = (None, "mixed", "bf16")
LENGTHS = (22, 300)


def query_grid():
    for L, (D, heads), hidden in mq.BLOCK:
        yield "stgcn_vit_block_forward_bf16_supported", (L, D, heads, hidden)
        yield "stgcn_vit_block_train_bf16_supported", (L, D, heads, hidden)
    for (M, K, N), ma, ti, ex in itertools.product(mq.LINEAR, mq.MATHS, mq.TILES, mq.EXTRA):
        yield "stgcn_vit_linear_bf16_supported", (M, K, N, ma | ti | ex)
    for M, K, N in mq.LINEAR:
        yield "stgcn_vit_linear_backward_bf16_supported", (M, K, N)
    for a in mq.ATTENTION:
        yield "stgcn_vit_attention_bf16_supported", a


def queries(handle):
    out = {}
    for q, args in query_grid():
        fn = getattr(handle, q)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_uint if (q == "stgcn_vit_linear_bf16_supported" and i == 3) else ctypes.c_int for i in range(len(args))]
        out.setdefault(q, []).append(int(fn(*args)))
    return out


def status_grid():
    """(flag word, block shape, pointers given) in a fixed order: 96 x 5 x 2."""
    return list(itertools.product(FLAGS, SHAPES, (False, True)))


def statuses(handle):
    """Per entry point, one record per case of ``status_grid()``: "<status>|<1 if the entry point's name is in the message>|
    <the TOKENS found, comma-separated>"."""
    P, S, I, U, FL = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_float
    proto = {"stgcn_vit_block_forward": [P] * 13 + [FL, FL, P, S, P] + [I] * 5 + [U, P],
             "stgcn_vit_block_forward_train": [P] * 15 + [FL, FL, P, S, P] + [I] * 5 + [U, P],
             "stgcn_vit_block_backward": [P] * 12 + [S] + [P] * 14 + [FL, FL, P, S] + [I] * 5 + [U, P],
             "stgcn_vit_linear_backward": [P] * 8 + [S] + [I] * 3 + [U, P]}
    for name, args in proto.items():
        getattr(handle, name).restype = ctypes.c_int
        getattr(handle, name).argtypes = args
    handle.stgcn_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 16)()           # never read or written: every case ends before a launch
    at = [ctypes.cast(ctypes.byref(buf, 8 * i), P) for i in range(4)]
    out = {e: [] for e in ENTRIES}
    for fl, (B, L, D, heads, hidden), given in status_grid():
        p, x, y, dy = at if given else [None] * 4
        dims = (B, L, D, heads, hidden, fl, None)
        calls = {"stgcn_vit_block_forward": (x, *[p] * 12, 1e-6, 0.1, p, 0, y, *dims),
                 "stgcn_vit_block_forward_train": (x, *[p] * 14, 1e-6, 0.1, p, 0, y, *dims),
                 "stgcn_vit_block_backward": (x, *[p] * 10, p, 0, dy, y, *[p] * 12, 1e-6, 0.1, p, 0, *dims),      # y's address as dx
                 "stgcn_vit_linear_backward": (dy, p, p, None, y, p, p, p, 0, *LINEAR_SHAPE, fl, None)}
        for e in ENTRIES:
            rc = getattr(handle, e)(*calls[e])
            msg = (handle.stgcn_last_error() or b"").decode()
            found = [t for t in TOKENS if (t in msg.lower() if t == "null" else t in msg)]
            out[e].append(f"{rc}|{int(e + ':' in msg)}|{','.join(found)}")
    return out


def flag_grid():
    """(math_mode, train_math_mode, STGCN_VIT_MATH, STGCN_VIT_TRAIN_MATH, small_tiles, L, training path) in a fixed order."""
    return list(itertools.product(MATH_MODES, TRAIN_MODES, ENV_MATH, ENV_TRAIN_MATH, (False, True), LENGTHS, (False, True)))


def block_flags():
    """The flag word that reaches the HIP path of each case of ``flag_grid()``, for one ``Block(64, 2)`` on CPU tensors."""
    import torch
    from stgcn_amd import altformer
    from stgcn_amd.altformer import HEAD_MATH, Block, set_head_math, set_train_math
    from stgcn_amd._capi import VIT_TILE_64, VIT_TILE_AUTO
    named = {"mixed|TILE_64": HEAD_MATH["mixed"] | VIT_TILE_64, "bf16|TILE_AUTO": HEAD_MATH["bf16"] | VIT_TILE_AUTO}
    seen = []

    class Recorder:
        @staticmethod
        def apply(x, s1, s2, heads, eps, scale, math, *params):
            seen.append(int(math))
            return x

    def forward_recorder(x, norm1, qkv, proj, norm2, fc1, fc2, heads, eps, scale, math=0):
        seen.append(int(math))
        return x
    keep = (altformer._BlockTrain, altformer.F.vit_block_forward, Block.uses_hip, Block.trains_on_hip,
            {k: os.environ.get(k) for k in ("STGCN_VIT_MATH", "STGCN_VIT_TRAIN_MATH")})
    altformer._BlockTrain, altformer.F.vit_block_forward = Recorder, forward_recorder
    try:
        torch.manual_seed(0)
        blk = Block(64, 2)
        xs = {L: torch.zeros(1, L, 64) for L in LENGTHS}
        for mode, tmode, env, tenv, small, L, train in flag_grid():
            set_head_math(blk, named.get(mode, mode))
            set_train_math(blk, tmode)
            blk.small_tiles = small
            for k, v in (("STGCN_VIT_MATH", env), ("STGCN_VIT_TRAIN_MATH", tenv)):
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            Block.uses_hip = lambda self, x, train=train: not train
            Block.trains_on_hip = lambda self, x, train=train: train
            n = len(seen)
            blk(xs[L])
            assert len(seen) == n + 1, "the call took neither HIP path"
    finally:
        altformer._BlockTrain, altformer.F.vit_block_forward, Block.uses_hip, Block.trains_on_hip, env0 = keep
        for k, v in env0.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return seen


def record(lib_path):
    handle = ctypes.CDLL(lib_path)
    return {"queries": queries(handle), "status": statuses(handle), "flags": block_flags()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "vit_plan_parent.json"))
    out = ap.parse_args().out
    from stgcn_amd import _capi
    got = record(_capi.LIB_PATH)
    with open(out, "w") as f:
        json.dump(got, f, separators=(",", ":"))
        f.write("\n")
    print(out, {k: len(v) for k, v in got["queries"].items()}, {k: len(v) for k, v in got["status"].items()}, len(got["flags"]))
