"""CPU test of the temporal conv's dispatch: the library's temporal-conv queries against tests/golden/tcn_dispatch.json.

Which kernel serves a shape, the size of the packed blob and the training workspaces that hold one are host decisions, all
read from one plan (csrc/tcn.hip).  The fixture (tests/golden/make_tcn_dispatch.py, which describes its layout) pins them
shape by shape over a grid of math modes and shapes; every figure but the kernel name was written by the library as it was
before that plan existed.
"""
import json
import os

from _util import GOLDEN

MATRIX_CORE = {"tcn_mfma_f32_kernel", "tcn_mfma_bf16_kernel", "tcn_bf16_v4_kernel", "tcn_bf16_v6_kernel"}
KERNELS = MATRIX_CORE | {"", "tcn_valu_kernel", "tcn_valu_joint_axis_kernel"}


def _shapes():
    """(flags name, flags, Cin, Cout, T, V, K, stride, packed_bytes, [supported, kernel name, 4 workspace sizes]) per shape."""
    with open(os.path.join(GOLDEN, "tcn_dispatch.json")) as fh:
        fx = json.load(fh)
    assert fx["ws_n"] == [2, 64] and fx["frozen_sizes"] == "equal"
    for sec in ("grid", "joint_axis"):
        for f, ci, co, K, s, packed, entries in fx[sec]["groups"]:
            assert len(entries) == len(fx[sec]["tv"])
            for (T, V), e in zip(fx[sec]["tv"], entries):
                yield f, fx["flag_sets"][f], ci, co, T, V, K, s, packed, [e[0], fx["kernels"][e[1]]] + e[2:]


def test_tcn_queries_match_dispatch_fixture():
    from stgcn_amd import _capi
    lib = _capi.lib()
    bad, n = [], 0
    for f, fl, ci, co, T, V, K, s, packed, want in _shapes():
        n += 1
        for frozen in (0, _capi.BN_FROZEN):      # every size was the same with STGCN_BN_FROZEN
            got = [lib.stgcn_tcn_supported(ci, co, T, V, K, s, fl), lib.stgcn_tcn_kernel_name(ci, co, T, V, K, s, fl).decode()]
            got += [fn(N, ci, co, T, V, K, s, fl | frozen) for fn in (lib.stgcn_tcn_train_ws_bytes, lib.stgcn_tcn_backward_ws_bytes)
                    for N in (2, 64)]
            if got != want or lib.stgcn_tcn_packed_bytes(ci, co, K, fl) != packed:
                bad.append(f"{(f, ci, co, T, V, K, s, frozen)}: want {packed} {want}\n      got  "
                           f"{lib.stgcn_tcn_packed_bytes(ci, co, K, fl)} {got}")
    assert n >= 4004
    assert not bad, f"{len(bad)} of {2 * n} queries differ:\n" + "\n".join(bad[:20])


def test_supported_means_a_matrix_core_kernel():
    shapes = list(_shapes())
    for sh in shapes:
        supported, kernel = sh[-1][:2]
        assert (supported == 1) == (kernel in MATRIX_CORE), sh
    assert {sh[-1][1] for sh in shapes} == KERNELS          # every kernel, and the refusal, occurs in the grid
    for f in ("f32", "bf16x3", "bf16"):                     # ... and both answers in every matrix-core mode
        assert {sh[-1][0] for sh in shapes if sh[0] == f} == {0, 1}


def test_joint_axis_goes_with_the_valu_mode_only():
    """STGCN_CONV_ALONG_V under any other math mode is refused by the forward call: no kernel, not supported."""
    from stgcn_amd import _capi
    lib = _capi.lib()
    for math in (_capi.MATH_F32, _capi.MATH_BF16X3, _capi.MATH_BF16):
        for (ci, co) in ((3, 64), (64, 128)):
            args = (ci, co, 12, 22, 9, 1, math | _capi.CONV_ALONG_V)
            assert lib.stgcn_tcn_kernel_name(*args) == b"" and lib.stgcn_tcn_supported(*args) == 0
