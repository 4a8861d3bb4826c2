"""Host only: ``ticket_point`` (voltrix/jit_kernels/spmm.py) -- which choices of ``spmm_kernel`` the ticket join's window launch can
run, and when its per-handle memo is dropped.  The tuner look-ups are stubbed: no device, no store file."""
import pytest
import torch

from voltrix import capi
from voltrix.jit_kernels import spmm as wrapper
from voltrix.jit_kernels.spmm import SCHED_PAIRS, SCHED_STREAM, SCHED_UNITS, ticket_point


@pytest.fixture
def tuner(monkeypatch):
    """``tuned``: hash tag -> point, what the stubbed tuner knows; the look-ups are counted in ``tuned["calls"]``."""
    tuned = {"calls": 0}

    def is_tuned(name, keys):
        tuned["calls"] += 1
        return name == "spmm_kernel" and keys["feature_hash"] in tuned

    monkeypatch.setattr(wrapper, "tuner_keys", lambda hspa_packed, embedding_dim, input, beside_panel, **kw: {
        "feature_hash": getattr(hspa_packed, "hash_tag", None), "embedding_dim": embedding_dim, "dtype": str(input.dtype),
        "two_level": bool(beside_panel)})
    monkeypatch.setattr(wrapper.jit_tuner, "is_tuned", is_tuned)
    monkeypatch.setattr(wrapper.jit_tuner, "tuned_point", lambda name, keys: tuned[keys["feature_hash"]])
    return tuned


def _handle(tag):
    hspa_packed = torch.zeros(4, dtype=torch.int32)
    hspa_packed.hash_tag = tag
    return hspa_packed


OPERAND = torch.zeros(16, 128, dtype=torch.float16)
GOOD = {"FS": 128, "DEPTH": 3, "WAVES": 4, "EB": 2, "SCHED": SCHED_PAIRS}


def test_none_before_the_first_spmm_kernel_call(tuner):
    handle = _handle("never_called")
    assert ticket_point(handle, 128, OPERAND, True) is None
    tuner["never_called"] = dict(GOOD)       # the first call has made the choice: not memoised as "none" for good
    assert ticket_point(handle, 128, OPERAND, True) == GOOD


@pytest.mark.parametrize("sched", [0, SCHED_UNITS, SCHED_PAIRS])
def test_the_points_the_library_can_run(tuner, sched):
    assert (128, 3, 4) in capi.tiles(True)
    tuner["good"] = dict(GOOD, SCHED=sched)
    point = ticket_point(_handle("good"), 128, OPERAND, True)
    assert point == dict(GOOD, SCHED=sched) and point is not tuner["good"]      # a copy: the caller may keep it


@pytest.mark.parametrize("change", [{"SCHED": SCHED_STREAM}, {"SCHED": 1}, {"EB": 4}, {"FS": 512}, {"DEPTH": 5}, {"WAVES": 3}],
                         ids=["stream-schedule", "window-order-schedule", "EB4", "FS512", "DEPTH5", "WAVES3"])
def test_none_for_points_the_ticket_launch_cannot_run(tuner, change):
    point = dict(GOOD, **change)
    if "SCHED" not in change and "EB" not in change:
        assert (point["FS"], point["DEPTH"], point["WAVES"]) not in capi.tiles(True)
    tuner["bad"] = point
    assert ticket_point(_handle("bad"), 128, OPERAND, True) is None


def test_memo_is_dropped_when_the_tuner_generation_changes(tuner, monkeypatch):
    handle = _handle("memo")
    tuner["memo"] = dict(GOOD)
    assert ticket_point(handle, 128, OPERAND, True) == GOOD
    calls = tuner["calls"]
    tuner["memo"] = dict(GOOD, FS=64)
    assert ticket_point(handle, 128, OPERAND, True) == GOOD and tuner["calls"] == calls         # the memo: no look-up
    assert ticket_point(handle, 64, OPERAND[:, :64], True) == dict(GOOD, FS=64)                # another width: another key
    monkeypatch.setattr(wrapper.jit_tuner, "generation", wrapper.jit_tuner.generation + 1)      # what jit_tuner.forget does
    assert ticket_point(handle, 128, OPERAND, True) == dict(GOOD, FS=64)
    handle.hash_tag = "memo_retagged"                                                           # ... and a new tag is a new handle
    assert ticket_point(handle, 128, OPERAND, True) is None
