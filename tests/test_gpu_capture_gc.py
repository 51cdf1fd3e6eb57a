"""GraphedStep keeps the cycle collector out of a stream capture (capture.py): dead engines and
probes are cyclic garbage holding captured graphs, and a graph finalised while another step is
being captured synchronises the device inside the capture.  Dead objects are collected before
the capture begins; the collector is off while it runs and back on afterwards."""
import gc

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Cycle:
    """Cyclic garbage with a visible finaliser."""

    def __init__(self, log):
        self.me, self.log = self, log

    def __del__(self):
        self.log.append("finalised")


def test_capture_runs_with_the_collector_off_and_garbage_gone():
    from avdino.capture import GraphedStep
    x = torch.zeros(8, device="cuda")
    seen, log = [], []

    def body():
        seen.append((gc.isenabled(), list(log)))
        x.add_(1.0)

    gs = GraphedStep(warmup=2)
    assert gc.isenabled()
    gs.run("k", body)
    gs.run("k", body)                 # two eager warm-up calls: the collector stays on
    assert [s[0] for s in seen] == [True, True]
    _Cycle(log)                       # dead at once, but only the cycle collector can free it
    gs.run("k", body)                 # the capture
    assert seen[2] == (False, ["finalised"])      # collected before the capture, collector off inside
    assert gc.isenabled() and gs.captures == 1
    gs.run("k", body)                 # a replay: the body is not called again
    torch.cuda.synchronize()
    assert len(seen) == 3 and x.tolist() == [4.0] * 8


def test_collector_stays_off_when_the_caller_had_it_off():
    from avdino.capture import GraphedStep
    x = torch.zeros(8, device="cuda")
    gc.disable()
    try:
        gs = GraphedStep(warmup=0)
        gs.run("k", lambda: x.add_(1.0))
        assert not gc.isenabled()     # the caller's choice is kept
    finally:
        gc.enable()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 8
