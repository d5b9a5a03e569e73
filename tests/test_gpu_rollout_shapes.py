"""GPU: swarm_rollout_record and swarm_rollout_sample (csrc/swarm_rollout.hip) past one grid pass
and at the segment counts and lengths tests/test_gpu_rollout_graph.py does not reach.

Both launches cap their grid at 8 workgroups per CU (`grid_for(..., 8)`); CAP_PER_CU mirrors that
constant and the CU count comes from the device properties, as tests/test_gpu_value.py mirrors its
grid.  Each test asserts on its sizes that the work exceeds one pass.

1. Record, second pass: one segment of 1.5 x cap tiles of 16 KiB plus 77 bytes (48 MiB on 256 CUs) at
   the three alignment classes (16-byte, 4-byte, byte) into a guard-filled arena, compared on the
   device.
2. Record, eight live segments of 16,383, 16,384, 16,385, 32,768, 16,400, 49,155, 1 and 65,536 bytes
   (a tile is 16,384 bytes: lengths one short of, exactly and one past a tile, whole multiples whose
   last tile is a full one, several tiles per segment) in three alignment mixes: every segment slot
   0..7 is selected.  Then the same eight with segments 0 and 3 skipped (dst NULL, zero bytes), which
   shifts the slot every later segment is packed into.  Every destination equals its source, every
   other byte of the arena is the guard, the sources are unchanged.
3. Sample, second pass: 1.5 x cap x 256 + 77 rows (786,509 on 256 CUs), act_dim 3 and 6, the counter
   split over the device word and the addend with a carry into the high word; the normals recovered
   from the actions against tests/policy_ref.py sample_noise64 over all rows under the bound of
   tests/test_gpu_policy_sample.py (derived in tests/test_gpu_policy_dims.py); rows r and r + one
   pass draw different normals; nothing past rows x act_dim is written.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import policy_ref as pr
from tests.test_gpu_policy_sample import check_z, recovered_z

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
CAP_PER_CU = 8        # grid_for(.., 8) of both launches
TILE = 16384          # TILE_BYTES of record_kernel
THREADS = 256         # rows per workgroup and pass of sample_kernel
GUARD = 0xA5
PAD = 256             # guard bytes around every destination
CLASSES = {"16B": (0, 0), "4B": (4, 8), "byte": (1, 2)}  # (src, dst) offsets from a 16-byte boundary


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _cap(dev):
    return CAP_PER_CU * torch.cuda.get_device_properties(dev).multi_processor_count


def _record(dev, rec):
    from swarm_marl_amd import _native as nat
    lib = nat.load_library()
    nat.check(lib.swarm_rollout_record(ctypes.byref(rec), torch.cuda.current_stream(dev).cuda_stream), lib, which="rollout")


def _tiles(nbytes):
    return -(-nbytes // TILE)


# ---------------------------------------------------------------- 1. record past one grid pass
@pytest.mark.parametrize("cls", list(CLASSES))
def test_record_walks_a_second_grid_pass(dev, cls):
    from swarm_marl_amd import _native as nat
    cap = _cap(dev)
    nbytes = (cap * 3 // 2) * TILE + 77
    assert _tiles(nbytes) > cap and _tiles(nbytes) < 2 * cap  # some workgroups take a second tile, some do not
    so, do = CLASSES[cls]
    g = torch.Generator(device=dev).manual_seed(len(cls))
    src = torch.randint(0, 256, (nbytes + 16,), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.full((nbytes + 2 * PAD,), GUARD, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and PAD % 16 == 0
    keep = src.clone()
    rec = nat.SwarmRolloutRecord()
    rec.count = 1
    rec.segments[0].src, rec.segments[0].dst, rec.segments[0].bytes = src.data_ptr() + so, dst.data_ptr() + PAD + do, nbytes
    _record(dev, rec)
    d0 = PAD + do
    assert torch.equal(dst[d0:d0 + nbytes], src[so:so + nbytes])
    assert bool((dst[:d0] == GUARD).all()) and bool((dst[d0 + nbytes:] == GUARD).all())
    assert torch.equal(src, keep)


# ---------------------------------------------------------------- 2. eight live segments
LENGTHS = (16383, 16384, 16385, 32768, 16400, 49152 + 3, 1, 65536)
# per mix, the alignment class of each segment: every length meets every class, and the exact
# multiples of a tile (segments 1, 3, 7) meet the 16-byte class, whose last tile is a whole one
MIXES = (
    ("byte", "16B", "4B", "16B", "byte", "4B", "16B", "16B"),
    ("16B", "4B", "byte", "4B", "16B", "byte", "4B", "byte"),
    ("4B", "byte", "16B", "byte", "4B", "16B", "byte", "4B"),
)


def _eight_segments(dev, mix, skipped=()):
    """One record call over LENGTHS in alignment mix `mix`; (got, want) host arenas."""
    from swarm_marl_amd import _native as nat
    span = [(n + 2 * PAD + 15) // 16 * 16 for n in LENGTHS]
    total = sum(span)
    g = torch.Generator(device=dev).manual_seed(7 + mix)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    host = src.cpu().numpy()
    want = np.full(total, GUARD, np.uint8)
    rec = nat.SwarmRolloutRecord()
    rec.count = len(LENGTHS)
    base = 0
    for i, (n, cls) in enumerate(zip(LENGTHS, MIXES[mix])):
        so, do = CLASSES[cls]
        s0, d0 = base + PAD + so, base + PAD + do
        seg = rec.segments[i]
        seg.src, seg.dst, seg.bytes = src.data_ptr() + s0, dst.data_ptr() + d0, n
        if i in skipped:  # the two ways to skip one
            if i % 2 == 0:
                seg.dst = None
            else:
                seg.bytes = 0
        else:
            want[d0:d0 + n] = host[s0:s0 + n]
        base += span[i]
    _record(dev, rec)
    got = dst.cpu().numpy()
    assert np.array_equal(src.cpu().numpy(), host)  # the sources are read only
    return got, want


@pytest.mark.parametrize("mix", [0, 1, 2])
def test_record_selects_every_one_of_eight_segments(dev, mix):
    from swarm_marl_amd import _native as nat
    assert len(LENGTHS) == nat.ROLLOUT_MAX_SEGMENTS == 8
    tiles = [_tiles(n) for n in LENGTHS]
    assert tiles == [1, 1, 2, 2, 2, 4, 1, 4] and sum(tiles) < _cap(dev)  # one pass: the segment select is what is new
    assert [n % TILE for n in LENGTHS].count(0) == 3 and sum(t > 1 for t in tiles) >= 4
    for i in range(8):  # every length meets every class, a whole last tile the 16-byte one among them
        assert {m[i] for m in MIXES} == set(CLASSES)
    got, want = _eight_segments(dev, mix)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_record_with_skipped_segments_among_eight(dev):
    """count = 8 with segment 0 (dst NULL) and segment 3 (zero bytes) skipped: segments 1 and 2 are
    packed into slots 0 and 1, segments 4..7 into slots 2..5."""
    got, want = _eight_segments(dev, 1, skipped=(0, 3))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    full_got, full_want = _eight_segments(dev, 1)
    assert np.array_equal(full_got, full_want) and not np.array_equal(full_want, want)  # the skipped ones stayed guard


# ---------------------------------------------------------------- 3. sample past one grid pass
@pytest.mark.parametrize("ad", [3, 6])
def test_sample_walks_a_second_grid_pass(dev, ad):
    from swarm_marl_amd import rollout_sample
    cap = _cap(dev)
    one_pass = cap * THREADS
    rows = one_pass * 3 // 2 + 77
    assert one_pass < rows < 2 * one_pass
    counter, word, add = (1 << 32) + 3, (1 << 32) - 2, 5  # the low word's carry goes into the high word
    assert word + add == counter and word < (1 << 32)
    rng = np.random.default_rng(ad)
    base = np.concatenate([rng.uniform(-1, 1, (pr.ROWS, ad)), rng.uniform(-2.0, 0.5, (pr.ROWS, ad))], axis=1).astype(np.float32)
    index = torch.arange(rows, device=dev) % pr.ROWS
    lg_dev = torch.from_numpy(base).to(dev)[index].contiguous()
    arena = torch.full((rows * ad + 64,), -555.0, device=dev)
    out = arena[:rows * ad].view(rows, ad)
    rollout_sample(lg_dev, out, seed=SEED, counter=add, counter_dev=torch.tensor([word], dtype=torch.int64, device=dev))
    assert bool((arena[rows * ad:] == -555.0).all())  # nothing past rows * ad is written
    a = out.cpu().numpy()
    lg = base[np.arange(rows) % pr.ROWS]
    z, ls = recovered_z(lg, a)
    check_z(z, pr.sample_noise64(rows, ad, SEED, counter), a, ls, f"swarm_rollout_sample rows={rows} ad={ad}")
    # the second pass draws from its own row index, not from the lane's
    later = z[one_pass:]
    assert len(later) == rows - one_pass and np.all(np.abs(later - z[:len(later)]).max(axis=1) > 1e-3)
