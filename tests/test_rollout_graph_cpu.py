"""CPU: the argument checks of csrc/swarm_rollout.hip's two entry points (no launch: every call
returns before touching the GPU), their struct layouts against the header, and the collector's
graph-mode refusals that need no device.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def _fails(nat, lib, rc, code, names=None):
    assert rc == getattr(nat, "SWARM_" + code), rc
    msg = lib.swarm_rollout_last_error()
    assert msg
    if names is not None:
        assert names in msg, msg
    with pytest.raises(ValueError, match="swarm_mi355x error"):
        nat.check(rc, lib, which="rollout")


def _sample(lib, logits=16, rows=4, act_dim=3, seed=1, counter_dev=64, counter_add=0, actions=128):
    return lib.swarm_rollout_sample(logits, rows, act_dim, seed, counter_dev, counter_add, actions, None)


@pytest.mark.parametrize("kw,code,names", [
    ({"logits": None}, "ENULL", None), ({"actions": None}, "ENULL", None),
    ({"act_dim": 0}, "ELIMIT", b"SWARM_ROLLOUT_MAX_ACT"), ({"act_dim": 7}, "ELIMIT", b"SWARM_ROLLOUT_MAX_ACT"),
    ({"act_dim": -1}, "ELIMIT", b"SWARM_ROLLOUT_MAX_ACT"), ({"rows": -1}, "EINVAL", b"rows"),
    ({"counter_dev": 68}, "EINVAL", b"8-byte"),
])
def test_sample_argument_errors(nat, lib, kw, code, names):
    _fails(nat, lib, _sample(lib, **kw), code, names)


def test_sample_empty_batch_is_a_no_op(nat, lib):
    assert _sample(lib, rows=0, logits=None, actions=None, counter_dev=None) == 0
    # the limits are checked first
    _fails(nat, lib, _sample(lib, rows=0, act_dim=7), "ELIMIT", b"SWARM_ROLLOUT_MAX_ACT")


def _record(nat, segs, count=None):
    r = nat.SwarmRolloutRecord()
    for i, (src, dst, nbytes) in enumerate(segs):
        r.segments[i].src, r.segments[i].dst, r.segments[i].bytes = src, dst, nbytes
    r.count = len(segs) if count is None else count
    return r


def test_record_argument_errors(nat, lib):
    assert lib.swarm_rollout_record(None, None) == nat.SWARM_ENULL
    _fails(nat, lib, lib.swarm_rollout_record(None, None), "ENULL")
    _fails(nat, lib, lib.swarm_rollout_record(ctypes.byref(_record(nat, [], count=9)), None), "ELIMIT",
           b"SWARM_ROLLOUT_MAX_SEGMENTS")
    _fails(nat, lib, lib.swarm_rollout_record(ctypes.byref(_record(nat, [], count=-1)), None), "EINVAL", b"count")
    _fails(nat, lib, lib.swarm_rollout_record(ctypes.byref(_record(nat, [(None, 32, 8)])), None), "ENULL", b"src")
    _fails(nat, lib, lib.swarm_rollout_record(ctypes.byref(_record(nat, [(16, 32, 2**46 + 1)])), None), "ELIMIT")


def test_record_with_nothing_to_copy_is_a_no_op(nat, lib):
    assert lib.swarm_rollout_record(ctypes.byref(_record(nat, [])), None) == 0
    # skipped segments: dst NULL (whatever src is) and zero bytes
    assert lib.swarm_rollout_record(ctypes.byref(_record(nat, [(None, None, 8), (16, 32, 0)] * 4)), None) == 0


@pytest.mark.parametrize("ctype,cname", [("SwarmRolloutSegment", "swarm_rollout_segment_t"),
                                         ("SwarmRolloutRecord", "swarm_rollout_record_t")])
def test_struct_layouts_match_header(nat, tmp_path, ctype, cname):
    cls = getattr(nat, ctype)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_mi355x.h"', "int main(void) {",
             f'printf("%zu\\n", sizeof({cname}));']
    lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines += ['printf("%d %d\\n", SWARM_ROLLOUT_MAX_SEGMENTS, SWARM_ROLLOUT_MAX_ACT);', "return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:-2] == [getattr(cls, f).offset for f in fields]
    assert out[-2:] == [nat.ROLLOUT_MAX_SEGMENTS, nat.ROLLOUT_MAX_ACT] == [8, 6]
    assert nat.ABI_VERSION == 5  # additions only


def test_symbols_are_bound(nat, lib):
    for name in nat.GRAPH_SYMBOLS:
        assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert nat.LAST_ERROR["rollout"] == "swarm_rollout_last_error"
    # the slices that name the other units still name them
    assert nat.ROLLOUT_SYMBOLS[0] == "swarm_critic_packed_bytes" and nat.PPO_SYMBOLS[-1] == "swarm_ppo_last_error"


def test_collector_takes_a_graph_argument():
    import inspect

    from swarm_marl_amd import RolloutCollector
    p = inspect.signature(RolloutCollector.__init__).parameters["graph"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_python_wrappers_check_before_any_launch():
    import torch

    from swarm_marl_amd import rollout_record, rollout_sample
    with pytest.raises(ValueError):
        rollout_sample(torch.zeros(4, 6), torch.zeros(4, 3))  # host tensors
    with pytest.raises(ValueError):
        rollout_record([(torch.zeros(4), torch.zeros(4))])
    with pytest.raises(ValueError, match="at most 8"):
        rollout_record([(None, None)] * 9)
    rollout_record([(None, None)] * 8)  # every pair skipped: no launch
