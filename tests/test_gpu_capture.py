"""GPU: graph.capture holds the collection guard — no cyclic garbage collection while the stream is capturing, the previous
state back afterwards, also when the captured callable raises (the stream then no longer captures and the library launches)."""

import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def test_collection_is_off_inside_a_capture_and_back_on_after_it(dev):
    from pytorch_generative_amd import graph, ops

    assert gc.isenabled()
    seen = []
    x = torch.ones(64, device=dev)
    graph.warm_up(lambda: ops.add(x, x))

    def step():
        seen.append((gc.isenabled(), torch.cuda.is_current_stream_capturing()))
        return ops.add(x, x)

    g, y = graph.capture(step)
    assert seen == [(False, True)] and gc.isenabled()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((64,), 2.0, device=dev))

    def failing():
        seen.append((gc.isenabled(), torch.cuda.is_current_stream_capturing()))
        ops.add(x, x)  # the capture is not empty when the step gives up, as a model's forward that raises half way
        raise RuntimeError("raised by the step")

    with pytest.raises(RuntimeError, match="raised by the step"):
        graph.capture(failing)
    assert seen[1] == (False, True) and gc.isenabled()
    assert not torch.cuda.is_current_stream_capturing()
    z = ops.zeros((5, 3), dev)  # a launch of the library after the failed capture
    torch.cuda.synchronize()
    assert torch.equal(z, torch.zeros(5, 3, device=dev))

    assert graph.try_capture([failing]) is None  # the optional form: None instead of the exception, same state afterwards
    assert gc.isenabled() and not torch.cuda.is_current_stream_capturing()
