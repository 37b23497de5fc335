"""GPU test of the packed blobs: SHA-256 of what stgcn_tcn_pack and stgcn_stem_prepare write, against
tests/golden/pack_digests.json.

The convolution and fused-stem kernels read these blobs at offsets the host plans (csrc/tcn.hip, csrc/stem.hip); the digests
were written by the library as it was before the temporal conv's plan existed, so they hold every byte and offset of both
blobs in place.  (They are also why the fused stem keeps its own pair-order pack kernel: with the temporal conv's, the three
bf16-mode stem blobs and f16mx's differ from these digests, a last bit of a lo value here and there.)
"""
import importlib.util
import json
import os

import pytest

from _util import GOLDEN


@pytest.mark.gpu
def test_packed_blobs_match_digests():
    from stgcn_amd import _capi
    spec = importlib.util.spec_from_file_location("make_pack_digests", os.path.join(GOLDEN, "make_pack_digests.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "pack_digests.json")) as fh:
        want = json.load(fh)
    assert len(want) == len(gen.TCN_CASES) + len(gen.STEM_CASES)
    got = gen.all_digests(_capi.lib())
    for name, (nbytes, digest) in got.items():
        print(f"{name:36s} {nbytes:9d} B  {digest}")
    assert got == want
