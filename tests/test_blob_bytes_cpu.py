"""CPU: every host packer's blob, byte for byte, against the hashes recorded before the blob formats
were gathered into csrc/swarm_nn.h (tests/golden/blob_sha256.json, written by tools/blob_hashes.py
from the library of that earlier commit).  The cases and the weights are tests/blob_cases.py's."""
from __future__ import annotations

import json

from tests import blob_cases
from tests.conftest import GOLDEN


def test_every_packed_blob_has_its_recorded_bytes():
    from swarm_marl_amd import _native as nat
    want = json.loads((GOLDEN / "blob_sha256.json").read_text())
    got = blob_cases.blob_hashes(nat.load_library(), nat)
    n = (len(blob_cases.POLICY_SHAPES) * len(blob_cases.POLICY_PRECISIONS)
         + (len(blob_cases.VALUE_INS) + len(blob_cases.CRITIC_INS) + len(blob_cases.ATTN_SHAPES))
         * len(blob_cases.TOWER_PRECISIONS))
    assert len(got) == n == 39 and set(got) == set(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_planted_values_are_the_intended_bit_patterns():
    """The generator's planted values land in the weights as written: NaNs keep their payloads
    through the float32 arrays, the bf16 ties are exact, and f32x3 gets no non-finite value."""
    import numpy as np
    w = blob_cases.mlp_weights("policy/in37_out6/bf16", 37, 6, "bf16")
    sp = blob_cases.specials("bf16")
    for arr, start in ((w[0], 7), (w[1], 3), (w[2], 5), (w[4], 11)):
        assert np.array_equal(arr.reshape(-1)[start:start + 7 * len(sp):7].view(np.uint32), sp.view(np.uint32))
    assert {0x7F800001, 0xFFC12345, 0x3F808000, 0x3F818000, 0x00000001} <= set(sp.view(np.uint32).tolist())
    x3 = blob_cases.specials("f32x3")
    assert np.all(np.isfinite(x3)) and np.abs(x3).max() < 65520 and np.float32(65504) in x3
    for a in blob_cases.mlp_weights("policy/in37_out6/f32x3", 37, 6, "f32x3"):
        assert np.all(np.isfinite(a)) and np.abs(a).max() < 65520
