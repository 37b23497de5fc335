"""Records what the host-side coverage queries of the ViT block answer, over the grid tests/test_altformer_bf16_host.py asks
again: tests/golden/vit_queries_abi11.json.  Run it on the library of the commit BEFORE the heads' bf16 mode (the fixture pins
that adding the mode changed no existing answer); needs no GPU.

    python tests/golden/make_golden_vit_queries.py path/to/libstgcn_hip.so
"""
import ctypes
import itertools
import json
import os
import sys

MATHS = (0, 1, 2, 3)                                    # f32, bf16x3, bf16, f32_valu in the low bits
TILES = (0, 0x10000, 0x20000, 0x30000)
EXTRA = (0, 0x2000)                                     # STGCN_VIT_QKV_F32
LINEAR = list(itertools.product((0, 1, 33, 200, 4096, 126720), (0, 32, 250, 256, 8192), (0, 1, 14, 96, 768)))
ATTENTION = list(itertools.product((0, 1, 22, 256, 257, 4096, 4097), (0, 8), (32, 48, 64)))
BLOCK = list(itertools.product((0, 1, 22, 46, 150, 180, 256, 257, 4096, 4097), ((256, 8), (512, 8), (384, 8), (256, 4), (8192, 128)),
                               (500, 512, 1024)))
BATCHES = (0, 1, 32, 3000)


def grid():
    """(query name, argument tuple) in a fixed order."""
    for (M, K, N), ma, ti, ex in itertools.product(LINEAR, MATHS, TILES, EXTRA):
        for q in ("stgcn_vit_linear_supported", "stgcn_vit_linear_tile", "stgcn_vit_linear_backward_supported"):
            yield q, (M, K, N, ma | ti | ex)
    for (M, K, N) in LINEAR:
        yield "stgcn_vit_linear_backward_ws_bytes", (M, K, N)
    for a in ATTENTION:
        for q in ("stgcn_vit_attention_supported", "stgcn_vit_attention_stream_supported", "stgcn_vit_attention_backward_supported",
                  "stgcn_vit_attention_backward_stream_supported"):
            yield q, a
    for L, (D, heads), hidden in BLOCK:
        for q in ("stgcn_vit_block_supported", "stgcn_vit_block_forward_supported", "stgcn_vit_block_train_supported",
                  "stgcn_vit_block_train_long_supported"):
            yield q, (L, D, heads, hidden)
        for B in BATCHES:
            for q in ("stgcn_vit_block_ws_bytes", "stgcn_vit_block_saved_bytes", "stgcn_vit_block_backward_ws_bytes",
                      "stgcn_vit_block_train_long_saved_bytes"):
                yield q, (B, L, D, hidden)
            yield "stgcn_vit_block_train_long_ws_bytes", (B, L, D, heads, hidden)


def answers(handle):
    out = {}
    for q, args in grid():
        fn = getattr(handle, q)
        fn.restype = ctypes.c_size_t if q.endswith("_bytes") else ctypes.c_int
        fn.argtypes = [ctypes.c_uint if (q.startswith("stgcn_vit_linear") and i == 3) else ctypes.c_int for i in range(len(args))]
        out.setdefault(q, []).append(int(fn(*args)))
    return out


if __name__ == "__main__":
    got = answers(ctypes.CDLL(sys.argv[1]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_queries_abi11.json")
    with open(path, "w") as f:
        json.dump(got, f, separators=(",", ":"))
    print(path, {k: len(v) for k, v in got.items()})
