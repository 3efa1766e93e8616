"""CPU: the host protocol the incremental samplers share — graph.no_gc (the collection guard of every capture), nn.Conv2d's
_row_clear, and ops.RowDecode's two walks over a model's modules."""

import gc

import pytest
import torch
from torch import nn


@pytest.fixture
def gc_state():
    was_on = gc.isenabled()
    yield
    (gc.enable if was_on else gc.disable)()


def test_no_gc_restores_the_previous_state(gc_state):
    from pytorch_generative_amd import graph

    gc.enable()
    with graph.no_gc():
        assert not gc.isenabled()
    assert gc.isenabled(), "collection was on before the guard and is not on after it"

    gc.disable()
    with graph.no_gc():
        assert not gc.isenabled()
    assert not gc.isenabled(), "collection was off before the guard: the guard must not switch it on"

    gc.enable()
    with pytest.raises(KeyError, match="inside"):
        with graph.no_gc():
            assert not gc.isenabled()
            raise KeyError("inside")
    assert gc.isenabled(), "an exception inside the guard left collection off"


def test_conv_row_clear_keeps_the_tensors():
    from pytorch_generative_amd import nn as pg_nn

    conv = pg_nn.Conv2d(3, 4, kernel_size=3, padding=1)
    conv._row_clear()  # nothing cached yet (no _row_reset either): nothing to do, no attribute appears
    assert getattr(conv, "_row_band", None) is None and getattr(conv, "_row_code_band", None) is None
    band, codes = torch.randn(2, 3, 2, 5), torch.rand(2, 1, 2, 5)
    conv._row_band, conv._row_code_band = band, codes
    conv._row_clear()
    assert conv._row_band is band and conv._row_code_band is codes
    assert torch.equal(band, torch.zeros(2, 3, 2, 5)) and torch.equal(codes, torch.full((2, 1, 2, 5), -1.0))
    conv._row_reset()
    assert conv._row_band is None and conv._row_code_band is None
    conv._row_clear()  # dropped caches: nothing to clear


class _Cached(nn.Module):
    def __init__(self, log, name, *children):
        super().__init__()
        self.log, self.name = log, name
        self.inner = nn.ModuleList(children)

    def _row_reset(self):
        self.log.append(("reset", self.name))

    def _row_clear(self):
        self.log.append(("clear", self.name))


class _ResetOnly(nn.Module):  # a cache that is never read past the current row (CausalAttention): no _row_clear
    def __init__(self, log, name):
        super().__init__()
        self.log, self.name = log, name

    def _row_reset(self):
        self.log.append(("reset", self.name))


def test_row_decode_walks_nested_modules_and_skips_those_without_hooks():
    from pytorch_generative_amd import ops

    log = []
    leaf, attn = _Cached(log, "leaf"), _ResetOnly(log, "attn")
    model = _Cached(log, "root", nn.Sequential(nn.ReLU(), _Cached(log, "mid", leaf)), nn.Linear(2, 2), attn)
    ops.RowDecode.drop_caches(model)
    assert log == [("reset", "root"), ("reset", "mid"), ("reset", "leaf"), ("reset", "attn")]  # modules() order, the model first
    del log[:]
    ops.RowDecode.clear_caches(model)
    assert log == [("clear", "root"), ("clear", "mid"), ("clear", "leaf")]
    del log[:]
    plain = nn.Sequential(nn.Linear(2, 2), nn.ReLU())
    ops.RowDecode.drop_caches(plain)
    ops.RowDecode.clear_caches(plain)
    assert log == []
