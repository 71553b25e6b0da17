"""mtp_amd.engine_base.EngineBase without a GPU: the order in which bursts of weight gradients are reported to on_block_done, and the freshness state of the
GEMM-side weight images.  The expected report orders are hand traces of the two loops BackboneEngine.backward / InternEngine.backward had of their own."""
import os
import re

import pytest
import torch

from conftest import ROOT
from mtp_amd import engine_base
from mtp_amd.engine_base import EngineBase


# ------------------------------------------------------------------------------------------------ burst reporter
class FakeQueue:
    """ops.WgradQueue as far as EngineBase uses it; `events` is shared with the test's on_block_done: ("launch" | "wait", burst) and ("report", group)"""
    events = None

    def __init__(self, stream=None):
        self.jobs, self.stream, self.launched, self.inflight = [], stream, 0, []
        self.max_jobs, self.sqn, self.covered = 0, None, []

    def should_flush(self):
        return bool(self.jobs)

    def flush(self):
        if not self.jobs:
            return
        self.jobs = []
        if self.stream is not None:
            self.launched += 1
            self.inflight.append(self.launched)
            self.events.append(("launch", self.launched))

    def wait(self, keep=0):
        while len(self.inflight) > keep:
            self.events.append(("wait", self.inflight.pop(0)))


class BurstEngine(EngineBase):
    wgrad_side_stream = True
    wgrad_max_jobs = 8
    wgrad_keep = 2

    def __init__(self, stream):
        super().__init__(None, torch.bfloat16)
        self._stream = stream

    def _wgrad_stream(self):
        return self._stream


def run_bursts(monkeypatch, stream, keep, tail, groups=(5, 4, 3, 2, 1, 0), empty=()):
    """six bursts, one per group (those in `empty` with nothing queued), then the tail of one engine -> (reported groups, events, group -> burst)"""
    events = []
    monkeypatch.setattr(FakeQueue, "events", events)
    monkeypatch.setattr(engine_base.ops, "WgradQueue", FakeQueue)
    eng = BurstEngine(stream)
    eng.wgrad_keep = keep
    sqn = object()
    wq = eng._begin_backward(sqn)
    assert wq is eng._wq and wq.sqn is sqn and eng.norm_covered is wq.covered and eng._ln_parts == [] and eng._sl_jobs == []
    assert wq.max_jobs == (8 if stream is not None else 0)
    done = lambda g: events.append(("report", g))
    burst_of = {}
    for g in groups:
        if g not in empty:
            wq.jobs.append(object())
        eng._burst_out(g, done)
        burst_of[g] = wq.launched
    if tail == "vit":            # BackboneEngine.backward: wait, the lowest pending group, [pos embed], -1
        eng._wait_bursts()
        eng._report_pending(done)
    else:                        # InternEngine.backward: the stem's burst, wait, -1
        wq.jobs.append(object())
        wq.flush()
        eng._ln_flush()
        eng._wait_bursts()
    done(-1)
    assert not wq.inflight
    return [g for kind, g in events if kind == "report"], events, burst_of


@pytest.mark.parametrize("tail", ["vit", "intern"])
def test_main_stream_mode_reports_every_group_at_once(monkeypatch, tail):
    order, events, _ = run_bursts(monkeypatch, None, 2, tail)
    assert order == [5, 4, 3, 2, 1, 0, -1]
    assert all(kind == "report" for kind, _ in events)       # nothing is launched aside, nothing is waited for


# keep -> (ViT, InternImage).  Burst n (group 6 - n) is launched, the current stream waits for all but the `keep` most recent bursts, and the groups of the
# bursts waited for are reported; ViT's tail waits for the rest and reports the lowest group of what was pending ONCE (it covers the others), InternImage's
# tail waits and reports the stem (-1) only.
SIDE_STREAM_ORDER = {
    0: ([5, 4, 3, 2, 1, 0, -1], [5, 4, 3, 2, 1, 0, -1]),       # every burst is waited for when it is launched: nothing is pending in the tail
    2: ([5, 4, 3, 2, 0, -1], [5, 4, 3, 2, -1]),                # bursts 3..6 wait for bursts 1..4; groups 1 and 0 are pending in the tail
    3: ([5, 4, 3, 0, -1], [5, 4, 3, -1]),                      # bursts 4..6 wait for bursts 1..3; groups 2, 1 and 0 are pending in the tail
}


@pytest.mark.parametrize("keep", [0, 2, 3])
@pytest.mark.parametrize("tail", ["vit", "intern"])
def test_side_stream_mode_report_order(monkeypatch, keep, tail):
    order, events, burst_of = run_bursts(monkeypatch, object(), keep, tail)
    assert order == SIDE_STREAM_ORDER[keep][tail == "intern"]
    for g in order[:-1]:          # never before the current stream has waited for the group's burst
        assert events.index(("wait", burst_of[g])) < events.index(("report", g)), (g, events)
    assert events.index(("wait", 6 if tail == "vit" else 7)) < events.index(("report", -1))
    # the two tails
    pending_at_tail = [g for g in (5, 4, 3, 2, 1, 0) if g not in order[:6 - keep]]
    assert order[6 - keep:] == (([min(pending_at_tail)] if pending_at_tail else []) + [-1] if tail == "vit" else [-1])


def test_a_burst_with_nothing_queued_is_reported_with_the_burst_before_it(monkeypatch):
    """BackboneEngine's `not wq.jobs` trigger (every weight gradient of the block went out immediately): no launch, the group takes the mark of the last one.
    keep = 2: call 3 waits for burst 1 -> 5; call 4 (group 2) launches nothing; call 5 = burst 4 waits for burst 2 -> 4; call 6 = burst 5 waits for
    burst 3 -> 3 and 2 (same mark); groups 1 and 0 pending in the tail."""
    order, events, burst_of = run_bursts(monkeypatch, object(), 2, "vit", empty=(2,))
    assert order == [5, 4, 3, 2, 0, -1]
    assert burst_of[2] == burst_of[3] == 3 and events.index(("wait", 3)) < events.index(("report", 2))


# ------------------------------------------------------------------------------------------------ weight-image cache
class CountingImages:
    def __init__(self, log):
        self.log = log

    def refresh(self):
        self.log.append("refresh")


class CacheEngine(EngineBase):
    images = True

    def __init__(self, module):
        super().__init__(module, torch.float32)
        self.log = []

    def _build_weight_images(self, P):
        self.log.append("build")
        self._wimg = CountingImages(self.log) if self.images else None

    def _fold_sources(self, P):
        self.log.append("fold")

    def _pack_weights(self, P):
        self.log.append("pack")

    def prepared(self, **kw):
        self.log.clear()
        self.prepare_weights(**kw)
        return list(self.log)


@pytest.fixture
def cache():
    eng = CacheEngine(torch.nn.Linear(4, 3))
    assert eng._key is None and eng._images_fresh is None and eng._wimg is None
    assert eng.prepared() == ["build", "fold", "refresh", "pack"]
    return eng


def touch(eng):
    with torch.no_grad():
        eng.m.weight.add_(0)


def test_unchanged_key_runs_no_hook(cache):
    assert cache.prepared() == []


def test_version_bump_refreshes_without_rebuild(cache):
    touch(cache)
    assert cache.prepared() == ["fold", "refresh", "pack"]
    assert cache.prepared() == []


def test_new_data_ptr_rebuilds(cache):
    cache.m.weight.data = cache.m.weight.data.clone()
    assert cache.prepared() == ["build", "fold", "refresh", "pack"]


def test_mark_images_fresh_skips_the_refresh_only(cache):
    cache.mark_images_fresh()
    assert cache.prepared() == ["fold", "pack"]          # the packed weights always follow
    assert cache._images_fresh is None
    assert cache.prepared() == []


def test_torch_edit_after_mark_images_fresh_refreshes(cache):
    cache.mark_images_fresh()
    touch(cache)
    assert cache.prepared() == ["fold", "refresh", "pack"]


def test_invalidate_after_mark_images_fresh_refreshes(cache):
    cache.mark_images_fresh()
    cache.invalidate_weights()
    assert cache._key is None and cache._images_fresh is None
    assert cache.prepared() == ["fold", "refresh", "pack"]


def test_force_refreshes_with_unchanged_key(cache):
    assert cache.prepared(force=True) == ["fold", "refresh", "pack"]
    cache.mark_images_fresh()
    assert cache.prepared(force=True) == ["fold", "refresh", "pack"]


def test_a_model_without_images_is_tolerated():
    """InternImage without an unpadded Linear: _build_weight_images leaves _wimg None -- no refresh, and no rebuild per call either"""
    eng = CacheEngine(torch.nn.Linear(4, 3))
    eng.images = False
    assert eng.prepared() == ["build", "fold", "pack"]
    assert eng.fusable_images() is None
    touch(eng)
    assert eng.prepared(force=True) == ["fold", "pack"]


def test_fusable_images(cache):
    assert cache.fusable_images() is cache._wimg


@pytest.mark.parametrize("attr", ["wgrad_side_stream", "wgrad_max_jobs", "wgrad_keep"])
def test_wgrad_options_are_per_engine_class(monkeypatch, attr):
    from mtp_amd.engine import BackboneEngine
    from mtp_amd.engine_intern import InternEngine
    assert issubclass(BackboneEngine, EngineBase) and issubclass(InternEngine, EngineBase)
    assert attr in vars(BackboneEngine) and attr in vars(InternEngine) and attr not in vars(EngineBase)
    before = (getattr(BackboneEngine, attr), getattr(InternEngine, attr))
    monkeypatch.setattr(BackboneEngine, attr, 17)
    assert getattr(InternEngine, attr) == before[1]
    monkeypatch.setattr(BackboneEngine, attr, before[0])
    monkeypatch.setattr(InternEngine, attr, 19)
    assert getattr(BackboneEngine, attr) == before[0]


def test_engine_defaults_stay():
    from mtp_amd.engine import BackboneEngine
    from mtp_amd.engine_intern import InternEngine
    assert (BackboneEngine.wgrad_side_stream, BackboneEngine.wgrad_max_jobs, BackboneEngine.wgrad_keep) == (True, 8, 2)
    assert (InternEngine.wgrad_side_stream, InternEngine.wgrad_max_jobs, InternEngine.wgrad_keep) == (2, 0, 3)


def test_the_trainer_pokes_no_private_engine_field():
    with open(os.path.join(ROOT, "mtp_amd", "parallel.py")) as f:
        src = f.read()
    assert re.findall(r"engine\._|co_varnames|hasattr\(self\.engine", src) == []
