"""GPU tests of training the ST-ViT head's two ends on HIP: ``stgcn_vit_patch_embed_backward`` and
``stgcn_vit_pool_classify_backward`` against fp64 autograd of the suite's restatements (tests/stvit_ends_ref.py), their optional
outputs, determinism, layouts, poisoned guard-banded buffers, the whole ``ViT`` against the reference's training fixture with
every piece on its HIP training branch, forward parity with the inference calls, and non-finite input.

Gates: the training tests' own (test_altformer_train_gpu.py): ``parity_gate`` at 1e-4, both criteria for 'f32' and 'mixed',
the max-norm criterion for 'bf16x3' (``TRAIN_STRICT``).  Every measured figure is printed before it is asserted."""
import pytest
import torch

import stvit_ends_ref as er
import stvit_ref as sr
import stvit_train_ref as vr
from _util import MATH_GATES, load_golden, parity_gate
from test_altformer_train_gpu import TRAIN_STRICT, gate_stored
from _util import HostileCase as Case, run_under_both_fills

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
LAYOUTS = ("nchw", "ntvc")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def _math(mode):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    return HEAD_TRAIN_MATH[mode]


_EMBED = {}


def embed_ref(name):
    """An embedding case, its dx and its fp64 gradients: made once per run and never changed."""
    if name not in _EMBED:
        N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
        z, W, bias, cls, pos = sr.embed_case(name)
        dx = er.make_dx(name)
        _EMBED[name] = dict(z=z, W=W, bias=bias, cls=cls, pos=pos, dx=dx, want=er.embed_grads64(z, W, bias, cls, pos, p1, p2, dx))
    return _EMBED[name]


def _layout(z, layout, dev):
    zd = z.to(dev)
    return zd if layout == "nchw" else zd.contiguous(memory_format=torch.channels_last)


def gate_embed(out, want, mode, what):
    for k in er.EMBED_OUTPUTS:
        err = (out[k].double().cpu() - want[k]).abs().max().item() / want[k].abs().max().item()
        print(f"{what} {k}: {err:.3e}")
    for k in er.EMBED_OUTPUTS:
        parity_gate(out[k], want[k], REL, f"{what} {k}", TRAIN_STRICT[mode])


# ---- 1. the embedding's backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(sr.EMBED_CASES))
def test_patch_embed_backward_vs_fp64(name, layout, mode, dev):
    from stgcn_amd import functional as F
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_ref(name)
    z = _layout(r["z"], layout, dev)
    W, dx = r["W"].to(dev), r["dx"].to(dev)
    assert F._is_channels_last(z) == (layout == "ntvc")
    out = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math(mode))
    print(f"{name} {layout} {mode}: cut {F.vit_patch_embed_backward_cut(N, C, T, V, p1, p2, E, _math(mode), layout == 'ntvc')}")
    assert out["dz"].shape == z.shape and out["dz"].stride() == z.stride(), "dz comes back in the layout of z"
    assert out["dW"].shape == W.shape and out["dpos"].shape == r["pos"].shape
    gate_embed(out, r["want"], mode, f"{name} {layout} {mode}")
    again = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math(mode))
    for k in er.EMBED_OUTPUTS:
        assert torch.equal(out[k], again[k]), f"{k}: two runs differ"


def test_the_cases_reach_two_token_splits_and_a_ragged_last_chunk():
    from stgcn_amd import functional as F
    rps, parts = F.vit_patch_embed_backward_cut(*sr.EMBED_CASES["d_rows396_tile128"])
    assert (rps, parts) == (224, 2) and (396 - rps) % 32 == 12
    assert F.vit_patch_embed_backward_cut(*sr.EMBED_CASES["a_K256_rows18"]) == (32, 1), "18 rows: less than one chunk"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["a_K256_rows18", "d_rows396_tile128"])
def test_each_output_is_optional_and_the_others_do_not_move(name, layout, dev):
    from stgcn_amd import functional as F
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_ref(name)
    z, W, dx = _layout(r["z"], layout, dev), r["W"].to(dev), r["dx"].to(dev)
    full = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math("bf16x3"))
    needs = {"dW": "need_dw", "dbias": "need_dbias", "dcls": "need_dcls", "dpos": "need_dpos", "dz": "need_dz"}
    for off in er.EMBED_OUTPUTS:
        out = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math("bf16x3"), **{needs[off]: False})
        assert out[off] is None
        for k in er.EMBED_OUTPUTS:
            assert k == off or torch.equal(out[k], full[k]), f"without {off}: {k} moved"
    only = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math("bf16x3"), need_dw=False, need_dcls=False, need_dpos=False, need_dz=False)
    assert torch.equal(only["dbias"], full["dbias"]), "dbias alone"
    # a frozen embedding still gives dz
    only = F.vit_patch_embed_backward(z, W, dx, p1, p2, _math("bf16x3"), need_dw=False, need_dbias=False, need_dcls=False, need_dpos=False)
    assert torch.equal(only["dz"], full["dz"])


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_the_two_layouts_agree_and_the_class_rows_reach_dcls_and_dpos_only(mode, dev):
    from stgcn_amd import functional as F
    name = "c_real_rows198"
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_ref(name)
    W, dx = r["W"].to(dev), r["dx"].to(dev)
    a = F.vit_patch_embed_backward(_layout(r["z"], "nchw", dev), W, dx, p1, p2, _math(mode))
    b = F.vit_patch_embed_backward(_layout(r["z"], "ntvc", dev), W, dx, p1, p2, _math(mode))
    assert a["dz"].is_contiguous() and F._is_channels_last(b["dz"])
    print(f"dz of the two layouts: {parity_gate(b['dz'], a['dz'], REL, 'dz ntvc against nchw', TRAIN_STRICT[mode]):.3e}")
    assert torch.equal(a["dz"], b["dz"]), "the same products in the same order, stored through one more pass"
    for k in ("dW", "dbias", "dcls", "dpos"):
        assert torch.equal(a[k], b[k]), k
    other = dx.clone()
    other[:, 0] = 3.0 * torch.randn(N, E, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) + 1.0
    c = F.vit_patch_embed_backward(_layout(r["z"], "ntvc", dev), W, other, p1, p2, _math(mode))
    for k in ("dW", "dbias", "dz"):
        assert torch.equal(c[k], b[k]), f"the class rows of dx moved {k}"
    assert not torch.equal(c["dcls"], b["dcls"]) and torch.equal(c["dpos"][1:], b["dpos"][1:])
    parity_gate(c["dcls"], other[:, 0].double().sum(0), REL, "dcls of the changed class rows")
    assert torch.equal(c["dcls"], c["dpos"][0])


def _small_model(dev, depth=2, **kw):
    from stgcn_amd import set_hip_min_tokens
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**dict(sr.CONFIG, depth=depth), dropout=0.1, emb_dropout=0.0, **kw)).to(dev)
    set_hip_min_tokens(model, 0)
    return model


def test_no_rearranged_copy_is_saved_for_the_backward(dev, monkeypatch):
    """The forward of ``ViT.embed`` on the HIP training branch saves no tensor of N n K elements but z itself; the torch branch
    saves the rearranged patches, which shows that the hook sees such a tensor."""
    model = _small_model(dev, depth=1).train()
    z = sr.make_input().to(dev).requires_grad_(True)
    N, n, K = sr.CLIPS, 99, 5120
    assert z.numel() == N * n * K

    def saved_big():
        seen = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (seen.append(t), t)[1], lambda t: t):
            x = model.embed(z)
        assert x.requires_grad
        return [t for t in seen if t.numel() == N * n * K]
    assert model.embed_trains_on_hip(z)
    big = saved_big()
    assert len(big) == 1 and big[0].data_ptr() == z.data_ptr() and big[0].shape == z.shape, [tuple(t.shape) for t in big]
    monkeypatch.setenv("STGCN_VIT_TRAIN_ENDS", "0")
    assert not model.embed_trains_on_hip(z)
    big = saved_big()
    assert any(t.data_ptr() != z.data_ptr() and t.numel() == N * n * K for t in big), "the torch branch keeps the rearranged copy"


# ---- 2. the classifier's backward -----------------------------------------------------------------------------------------------------
_CLASSIFY = {}


def classify_ref(name, pool):
    if (name, pool) not in _CLASSIFY:
        t = er.classify_case(name)
        _CLASSIFY[name, pool] = (t, er.classify_grads64(*t, pool))
    return _CLASSIFY[name, pool]


@pytest.mark.parametrize("pool", ["cls", "mean"])
@pytest.mark.parametrize("name", sorted(er.CLASSIFY_CASES))
def test_pool_classify_backward_vs_fp64(name, pool, dev):
    from stgcn_amd import functional as F
    (x, ln_w, ln_b, W, bias, dl), (logits, want) = classify_ref(name, pool)
    xd, wd, bd, Wd, biasd, dld = (t.to(dev) for t in (x, ln_w, ln_b, W, bias, dl))
    parity_gate(F.vit_pool_classify(xd, wd, bd, sr.LN_EPS, Wd, biasd, mode=pool), logits, REL, f"{name} {pool} logits")
    out = F.vit_pool_classify_backward(xd, wd, bd, sr.LN_EPS, Wd, dld, mode=pool)
    for k in er.CLASSIFY_OUTPUTS:
        print(f"{name} {pool} {k}: {(out[k].double().cpu() - want[k]).abs().max().item() / want[k].abs().max().item():.3e}")
    for k in er.CLASSIFY_OUTPUTS:
        parity_gate(out[k], want[k], REL, f"{name} {pool} {k}")
    if pool == "cls":
        assert not out["dx"][:, 1:].any(), "rows 1 .. L - 1 of dx are exactly zero"
    else:
        assert torch.equal(out["dx"], out["dx"][:, :1].expand_as(out["dx"])), "every row gets the pooled gradient / L"
    again = F.vit_pool_classify_backward(xd, wd, bd, sr.LN_EPS, Wd, dld, mode=pool)
    assert all(torch.equal(out[k], again[k]) for k in er.CLASSIFY_OUTPUTS), "two runs differ"
    # each output optional, the others unmoved
    for off, kw in (("dx", dict(need_dx=False)), ("dln_weight", dict(need_dln=(False, True))), ("dln_bias", dict(need_dln=(True, False))),
                    ("dW", dict(need_dw=False)), ("dbias", dict(need_dbias=False))):
        part = F.vit_pool_classify_backward(xd, wd, bd, sr.LN_EPS, Wd, dld, mode=pool, **kw)
        assert part[off] is None and all(k == off or torch.equal(part[k], out[k]) for k in er.CLASSIFY_OUTPUTS), off


def test_the_max_pool_has_no_backward(dev):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    (x, ln_w, ln_b, W, bias, dl), _ = classify_ref("small", "cls")
    with pytest.raises(_capi.StgcnError) as e:
        F.vit_pool_classify_backward(*(t.to(dev) for t in (x, ln_w, ln_b)), sr.LN_EPS, W.to(dev), dl.to(dev), mode="max")
    assert e.value.code == -2 and "STGCN_VIT_POOL_MAX" in str(e.value)


# ---- 3. poisoned, guard-banded buffers ------------------------------------------------------------------------------------------------
def make_embed_case(name, layout, mode, dev):
    from stgcn_amd import functional as F
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_ref(name)
    z, W, dx = _layout(r["z"], layout, dev), r["W"].to(dev), r["dx"].to(dev)
    return (lambda: F.vit_patch_embed_backward(z, W, dx, p1, p2, _math(mode))), (lambda o, what: gate_embed(o, r["want"], mode, what))


def make_classify_case(name, pool, dev):
    from stgcn_amd import functional as F
    t, (_, want) = classify_ref(name, pool)
    xd, wd, bd, Wd, _, dld = (v.to(dev) for v in t)

    def gate(o, what):
        for k in er.CLASSIFY_OUTPUTS:
            parity_gate(o[k], want[k], REL, f"{what} {k}")
        assert pool != "cls" or not o["dx"][:, 1:].any()
    return (lambda: F.vit_pool_classify_backward(xd, wd, bd, sr.LN_EPS, Wd, dld, mode=pool)), gate


BUFFER_CASES = [Case(f"vit_patch_embed_backward-{n}-{l}-{m}", lambda dev, n=n, l=l, m=m: make_embed_case(n, l, m, dev), True)
                for n, l, m in (("a_K256_rows18", "nchw", "f32"), ("a_K256_rows18", "ntvc", "bf16x3"),
                                ("d_rows396_tile128", "nchw", "bf16x3"), ("d_rows396_tile128", "ntvc", "f32"))] + \
               [Case(f"vit_pool_classify_backward-{n}-{p}", lambda dev, n=n, p=p: make_classify_case(n, p, dev), True)
                for n, p in (("small", "cls"), ("real", "cls"), ("real", "mean"))]


@pytest.mark.parametrize("case", BUFFER_CASES, ids=lambda c: c.id)
def test_both_backwards_under_poisoned_guard_banded_buffers(case, dev):
    run_under_both_fills(case, dev)


# ---- 4. the whole model against the reference's training fixture ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_model(dev):
    ref = load_golden("stvit_train_reference")
    depth = int(ref["depth"])
    assert depth == vr.FIXTURE_DEPTH == 2
    model = _small_model(dev, depth=depth).train()
    for i, layer in enumerate(model.transformer.layers):       # the fixture's masks in place of the generator's
        masks = tuple(m.to(dev) for m in vr.fixture_masks(i))
        layer.draw_dropout = lambda x, masks=masks: masks
    return model, ref


@pytest.mark.parametrize("ends", ["hip", "torch"])
@pytest.mark.parametrize("mode", ["f32", "mixed"])
def test_whole_vit_trains_against_the_reference_fixture(mode, ends, fixture_model, dev, monkeypatch):
    import stgcn_amd
    model, ref = fixture_model
    if ends == "torch":
        monkeypatch.setenv("STGCN_VIT_TRAIN_ENDS", "0")
    stgcn_amd.set_train_math(model, mode)
    try:
        for p in model.parameters():
            p.grad = None
        z = sr.make_input().to(dev).requires_grad_(True)
        took = {}
        real_embed, real_classify = model.embed, model.classify
        model.embed = lambda t: (took.__setitem__("embed", model.embed_trains_on_hip(t)), real_embed(t))[1]
        model.classify = lambda t: (took.__setitem__("head", model.head_trains_on_hip(t)), real_classify(t))[1]
        hooks = [l.register_forward_pre_hook(lambda mod, args: took.setdefault("layers", []).append(mod.trains_on_hip(args[0])))
                 for l in model.transformer.layers]
        try:
            logits = model(z)
        finally:
            del model.embed, model.classify
            for h in hooks:
                h.remove()
        assert took == {"embed": ends == "hip", "layers": [True, True], "head": ends == "hip"}, took
        logits.backward(vr.fixture_dlogits().to(dev))
    finally:
        stgcn_amd.set_train_math(model, None)
    strict = TRAIN_STRICT[mode]
    what = f"whole ViT {mode} ends={ends}"
    gate_stored(logits.detach(), ref, "logits", f"{what} logits", strict)
    gate_stored(z.grad, ref, "dz", f"{what} dz", strict)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert {"d" + k for k in grads} | {"dz"} == {k[:-len("_absmax")] for k in ref if k.endswith("_absmax")}
    for k, g in grads.items():
        assert g is not None, k
        gate_stored(g, ref, "d" + k, f"{what} d{k}", strict)


# ---- 5. forward parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "mixed", "bf16"])
def test_the_forward_of_a_recorded_call_is_the_inference_call(mode, dev):
    import stgcn_amd
    from stgcn_amd import functional as F
    model = _small_model(dev, depth=1).train()
    stgcn_amd.set_train_math(model, mode)
    pat, lin = model.to_patch_embedding
    ln, head = model.mlp_head
    for layout in LAYOUTS:
        z = _layout(sr.make_input(), layout, dev).requires_grad_(True)
        assert model.embed_trains_on_hip(z) and not model.embed_on_hip(z)
        x = model.embed(z)
        assert x.requires_grad and model.head_trains_on_hip(x)
        with torch.no_grad():
            assert torch.equal(x, F.vit_patch_embed(z, lin.weight, lin.bias, model.cls_token, model.pos_embedding[0, :100], pat.p1,
                                                    pat.p2, model._train_flags()))
        for pool in ("cls", "mean"):
            model.pool = pool
            logits = model.classify(x)
            assert logits.requires_grad
            with torch.no_grad():
                assert torch.equal(logits, F.vit_pool_classify(x, ln.weight, ln.bias, ln.eps, head.weight, head.bias, mode=pool))


# ---- 6. non-finite input --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_nan_in_one_clips_dx_stays_out_of_the_other_clips_dz(layout, dev):
    from stgcn_amd import functional as F
    name = "d_rows396_tile128"
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_ref(name)
    z, W = _layout(r["z"], layout, dev), r["W"].to(dev)
    bad = r["dx"].clone()
    bad[2, 57, 300] = float("nan")
    clean = F.vit_patch_embed_backward(z, W, r["dx"].to(dev), p1, p2, _math("bf16x3"))
    out = F.vit_patch_embed_backward(z, W, bad.to(dev), p1, p2, _math("bf16x3"))
    assert torch.isnan(out["dz"][2]).any(), "the clip that holds the NaN"
    for i in (0, 1, 3):
        assert torch.equal(out["dz"][i], clean["dz"][i]), f"the NaN of clip 2 moved dz of clip {i}"
    want = er.embed_grads64(r["z"], r["W"], r["bias"], r["cls"], r["pos"], p1, p2, bad)
    for k in ("dW", "dbias", "dpos"):
        assert not torch.isfinite(want[k]).all() and not torch.isfinite(out[k]).all(), f"{k} is non-finite, as the reference's"
        assert torch.equal(torch.isfinite(out[k]).cpu(), torch.isfinite(want[k])), f"{k}: non-finite where the reference's is"
    assert torch.isfinite(out["dcls"]).all() and torch.isfinite(want["dcls"]).all(), "row 57 is no class row"
