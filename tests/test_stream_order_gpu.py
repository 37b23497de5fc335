"""GPU tests of the stream contract ("Streams"; the table and the helpers are tests/stream_order.py): every HIP entry
point orders all its work on the stream it is given, waits for nothing on the host, and can be captured into a graph.

1. ``test_late_input_behind_a_held_stream``: per case, two calls and a late input enqueued behind a held side stream
   (stream_order.held_run); the second result is held to the fp64 reference of the clean input with the case's own gates.
   The enqueue time, the hold and ``hold_end.query()`` are printed.  The library symbols the case really calls are recorded by
   a proxy round the loaded library for the duration of the case (stream_order.Recorder; stgcn_amd/_capi.py is unchanged) and
   compared with the case's declaration, which tests/test_stream_order_host.py holds against the header.
2. ``test_replay_under_a_new_input``: for the paths no other test captures - a graph captured on a side stream while the input
   holds the decoy, replayed once after the clean input was copied in.  It catches a value read on the host and baked into the
   launch arguments, and an allocation the replay no longer owns.  A case runs it only after it passed 1 in this session
   (a stray launch during capture is an error): otherwise it fails, naming that.
3. ``test_the_control_pipeline_fails_off_stream``: the helper of 1 on two torch ops - both on the side stream (passes), the
   second under the default stream on purpose (the helper reports the mismatch).  No library kernel, nothing that can fault."""
import functools

import pytest
import torch

import stream_order as so

pytestmark = pytest.mark.gpu
PASSED_HELD = set()               # ids that passed test 1 in this session
_STAGED = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hold(dev):
    h = so.Hold(dev)
    print(f"hold: one {so.HOLD_N}^3 fp32 matmul takes {h.matmul_ms:.3f} ms; {h.count} of them for {h.ms:.0f} ms")
    return h


@functools.lru_cache(maxsize=None)
def clean_reference(case):
    """reference(clean), once per case and never changed."""
    prep = case.prepare()
    return prep.reference(prep.x)


def staged(case, dev):
    if case.id not in _STAGED:
        clean_reference(case)                       # a kink-free cotangent comes from the clean reference: before staging
        _STAGED[case.id] = case.prepare().on(dev)
    return _STAGED[case.id]


@pytest.mark.parametrize("case", so.CASES, ids=lambda c: c.id)
def test_late_input_behind_a_held_stream(case, dev, hold):
    prep, ref, run = case.prepare(), clean_reference(case), staged(case, dev)
    with so.Recorder() as rec:
        out = so.held_run(run, prep.x, dev, hold, case.id)
    called = rec.names & set(so.stream_entry_points())
    print(f"{case.id}: calls {sorted(called)}")
    bad = so.mismatches(case, prep, out, ref, case.id)
    assert not bad, f"{case.id}: the result behind the held stream is not that of the clean input: " + "; ".join(bad)
    assert case.symbols <= called and called - case.symbols <= so.STAGING, f"{case.id}: declared {sorted(case.symbols)}, called {sorted(called)}"
    PASSED_HELD.add(case.id)


@pytest.mark.parametrize("case", [c for c in so.CASES if c.replay], ids=lambda c: c.id)
def test_replay_under_a_new_input(case, dev):
    if case.id not in PASSED_HELD:
        pytest.fail(f"{case.id} did not pass test_late_input_behind_a_held_stream in this session: not captured")
    prep, ref, run = case.prepare(), clean_reference(case), staged(case, dev)
    clean_dev = prep.x.to(dev)
    xd = so.decoy(prep.x).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(xd.detach())
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = run(xd.detach())
    with torch.no_grad():
        xd.copy_(clean_dev)
    torch.cuda.synchronize(dev)
    g.replay()
    torch.cuda.synchronize(dev)
    bad = so.mismatches(case, prep, out, ref, f"{case.id} replayed")
    assert not bad, f"{case.id}: the replay under the clean input is not its result: " + "; ".join(bad)
    del g


class _Control:
    """y = x * 2 then z = y + 1 into buffers made beforehand; ``stray``: the second op goes to the default stream."""
    id, no_dependence = "control", {}

    def __init__(self, dev, stray):
        self.x = torch.randn(64, 1024, generator=torch.Generator().manual_seed(3))
        self.y, self.z = torch.empty(64, 1024, device=dev), torch.empty(64, 1024, device=dev)
        self.dev, self.stray = dev, stray

    def gate_of(self, prep, name):
        return (1e-6, True)          # two exact fp32 operations on values of a few units: the fp64 reference rounds to the same

    def reference(self, x):
        return {"z": x.double() * 2 + 1}

    def run(self, x):
        torch.mul(x, 2.0, out=self.y)
        if self.stray:
            with torch.cuda.stream(torch.cuda.default_stream(self.dev)):
                torch.add(self.y, 1.0, out=self.z)
        else:
            torch.add(self.y, 1.0, out=self.z)
        return {"z": self.z}


def test_the_control_pipeline_fails_off_stream(dev, hold):
    for stray in (False, True):
        c = _Control(dev, stray)
        out = so.held_run(c.run, c.x, dev, hold, f"control stray={stray}")
        bad = so.mismatches(c, None, out, c.reference(c.x), f"control stray={stray}")
        print(f"control stray={stray}: {len(bad)} mismatch(es) {bad}")
        if stray:
            assert bad, "the second op ran on the default stream, ahead of its producer, and the helper did not notice"
        else:
            assert not bad, "both ops on the side stream: " + "; ".join(bad)
