"""CPU test of the graph conv's dispatch: stgcn_agcn_attention_kernel_name and stgcn_agcn_expand_kernel_name against
tests/golden/agcn_dispatch.json, the kernel trace of the commit before both choices moved behind one plan each (csrc/agcn.hip;
tests/golden/make_agcn_digests.py has the cases and wrote the fixture), and against the fused stem's queries over a dense grid.
No pointer is passed to any entry point: nothing can launch."""
import importlib.util
import json
import os

from _util import GOLDEN

_spec = importlib.util.spec_from_file_location("make_agcn_digests", os.path.join(GOLDEN, "make_agcn_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

CIN = list(range(1, 9)) + [16, 64, 128, 256, 260]
INTER_C = (8, 16, 32, 64, 1024)
SUBSETS = (1, 3, 4)
BF16X3 = 1


def _lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_name_queries_match_the_traced_dispatch():
    lib = _lib()
    with open(os.path.join(GOLDEN, "agcn_dispatch.json")) as fh:
        fx = json.load(fh)
    cases = mk.cases()
    assert set(fx["cases"]) == {c["id"] for c in cases} and fx["commit"]
    seen = set()
    for c in cases:
        e = fx["cases"][c["id"]]
        att, exp = mk.queries(c, lib)
        assert [list(att), [list(q) for q in exp]] == [e["attention_query"], e["expand_queries"]], c["id"]
        traced = [d[0] for d in e["dispatches"]]
        seen.update(traced)
        want_att = [n for n in traced if n.startswith("attention_")]
        want_exp = [n for n in traced if n.startswith("agcn_expand_")]
        got = lib.stgcn_agcn_attention_kernel_name(*att).decode()
        assert [got] == want_att or (got == "" and not traced), (c["id"], got, traced)
        assert [lib.stgcn_agcn_expand_kernel_name(*q).decode() for q in exp] == want_exp, (c["id"], traced)
    assert set(mk.KERNELS) <= seen, "every kernel and instantiation of both plans occurs in the trace"
    refused = [k for k, v in fx["cases"].items() if not v["dispatches"]]
    assert len(refused) == 2 and all(k.startswith("attention-") for k in refused)


def test_queries_over_a_dense_grid():
    """Where the fused stem asks the attention for features (stgcn_stem_features_used, any C, T and math mode of the grid),
    ``extra = 1`` names a folded form, and it names one inside the stem class only.  The converse does not hold and is not
    asserted: the stem takes features at some V and T only (fragments at V = 22 and on even wide frames, nothing above
    V = 48), while the attention can emit them for every V up to 51."""
    lib = _lib()
    att, exp, feat = lib.stgcn_agcn_attention_kernel_name, lib.stgcn_agcn_expand_kernel_name, lib.stgcn_stem_features_used
    known, bad, n = set(mk.KERNELS) | {""}, [], 0
    for Cin in CIN:
        for V in range(1, 71):
            for S in SUBSETS:
                stem = {(C, T, fl): feat(Cin, C, T, V, 9, S, fl) for C in (64, 128, 256) for T in (1, 8, 40, 300)
                        for fl in (0, BF16X3, 2, BF16X3 | 0x400)}
                # (T does not enter attention_emits_features, csrc/agcn.hip: the stem's answer at inter_c = 32 is the query's)
                emits = {att(2, Cin, T, V, 32, S, 1).decode() for T in (1, 8, 40, 300, 1 << 20)}
                assert len(emits) == 1, (Cin, V, S, emits)
                emits = emits.pop()
                if any(stem.values()) and not emits.startswith("attention_folded_kernel<"):
                    bad.append(("stem features without a folded form", Cin, V, S, emits))
                if emits and not (Cin == 3 and S == 3 and V <= 64):
                    bad.append(("features outside the stem class", Cin, V, S, emits))
                for ic in INTER_C:
                    names = [att(2, Cin, 8, V, ic, S, x).decode() for x in range(4)]
                    n += 4       # (V <= 64 is served whenever a frame of x and both embeddings fits LDS: every ic <= 64 here)
                    if not set(names) <= known or (V > 64 and any(names)) or (V <= 64 and ic <= 64 and not names[0]):
                        bad.append(("attention", Cin, V, ic, S, names))
                    if any(nm and not nm.startswith("attention_folded_kernel<") for nm in names[1:]):
                        bad.append(("an extra output from a generic form", Cin, V, ic, S, names))
                for Cout in (Cin, 64, 128, 256):
                    for down in (0, 1):
                        nm = exp(2, Cin, Cout, 8, V, S, down).decode()
                        n += 1
                        if nm not in known or nm.startswith("attention") or (nm.startswith("agcn_expand_small") and not (Cin == 3 and S == 3 and down)):
                            bad.append(("expand", Cin, Cout, V, S, down, nm))
    assert n == len(CIN) * 70 * len(SUBSETS) * (4 * len(INTER_C) + 8)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(map(str, bad[:20]))
    for q in (att, exp):                      # the 16-bit grid limit, and nonsense arguments
        assert q(65535, 3, 128 if q is exp else 8, 8, 22, 3, 0 if q is att else 1) != b"" and q(0, 3, 8, 8, 22, 3, 0) == b""
    assert att(65536, 3, 8, 22, 32, 3, 0) == b"" and exp(65536, 3, 128, 8, 22, 3, 1) == b"" and att(2, 3, 8, 22, 32, 3, 4) == b""
