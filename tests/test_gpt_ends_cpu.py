"""Host side of ImageGPT's fused ends (csrc/gpt_ends.hip, ops/gpt_ends.py): the launch plans the workspaces are sized by, the
chain's bookkeeping and the predicates that route ImageGPT.forward. No GPU."""

import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from pytorch_generative_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (5, 28, 28), (64, 28, 28), (1024, 28, 28), (3, 64, 64)])
@pytest.mark.parametrize("cap", [0, 1, 2, 3, 100])
def test_stem_backward_plan(lib, n, h, w, cap):
    rows, slices = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.pg_gpt_stem_bwd_plan(n, h, w, cap, ctypes.byref(rows), ctypes.byref(slices)) == 0
    chunks = (h * w + 127) // 128  # positions per tile: at most 128
    assert 1 <= slices.value <= n and 1 <= rows.value <= chunks * slices.value
    assert rows.value <= (cap or 1024)
    if cap == 0 and chunks * slices.value <= 1024:
        assert rows.value == chunks * slices.value  # one tile per workgroup
    assert lib.pg_gpt_stem_bwd_workspace_floats(n, h, w, cap) == rows.value * 160 + slices.value * 4 * h * w


@pytest.mark.parametrize("n,L,cap,want", [(1, 1, 0, 1), (2, 35, 0, 1), (5, 784, 0, 4), (5, 784, 3, 3), (5, 784, 1, 1),
                                          (1024, 784, 0, 784), (4096, 784, 0, 2048)])
def test_output_head_backward_rows(lib, n, L, cap, want):
    assert lib.pg_gpt_out_head_bwd_rows(n, L, cap) == want  # ceil(N L / 1024) tiles, at most grid_cap (default 2048) workgroups


def test_bad_arguments_are_refused(lib):
    rows, slices = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.pg_gpt_stem_bwd_plan(0, 4, 4, 0, ctypes.byref(rows), ctypes.byref(slices)) != 0
    assert lib.pg_gpt_stem_bwd_plan(2, 4, 4, -1, ctypes.byref(rows), ctypes.byref(slices)) != 0
    assert lib.pg_gpt_stem_bwd_workspace_floats(2, 0, 4, 0) == 0 and lib.pg_gpt_out_head_bwd_rows(2, 16, -1) == 0
    # nothing to reduce, more than 8 blocks, an end without destinations
    assert lib.pg_gpt_model_reduce(0, None, None, None, 2, 16, 16, 0, 0, 0, None, 0, 0, 0, 0, 0, None, 0) != 0
    assert lib.pg_gpt_model_reduce(9, None, None, None, 2, 16, 16, 0, 0, 0, None, 0, 0, 0, 0, 0, None, 0) != 0
    assert lib.pg_gpt_model_reduce(0, None, None, None, 2, 16, 16, 4096, 1, 1, None, 0, 0, 0, 0, 0, None, 0) != 0
    assert lib.pg_gpt_out_head_fwd(4096, 4096, 4096, 4096, 4096, 4096, 2, 16, 5, 16, 1e-5, 0, 0) != 0  # Cout > 4
    assert lib.pg_gpt_out_head_fwd(4096, 4096, 4096, 4096, 4096, 4096, 2, 8, 1, 16, 1e-5, 0, 0) != 0   # C != 16


def test_parked_output_head_rows_count_as_pending():
    from pytorch_generative_amd import ops

    chain = ops.new_block_chain()
    ops.assert_no_pending_block_reductions()
    chain.out = ("workspace", 1, 1, [])
    with pytest.raises(RuntimeError, match="never flushed"):
        ops.assert_no_pending_block_reductions()
    chain.out = None
    ops.assert_no_pending_block_reductions()


def test_predicates_route_only_the_baseline_shapes():
    from pytorch_generative_amd import nn as pg_nn, ops

    conv = pg_nn.CausalConv2d(True, in_channels=1, out_channels=16, kernel_size=3, padding=1)
    pos, img = torch.zeros(1, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    assert not ops.gpt_stem_supported(img, pos, conv)  # a CPU tensor: the generic path raises its own error
    meta = torch.empty(2, 1, 8, 8, device="meta")
    for bad in (pg_nn.CausalConv2d(False, in_channels=1, out_channels=16, kernel_size=3, padding=1),
                pg_nn.CausalConv2d(True, in_channels=1, out_channels=32, kernel_size=3, padding=1),
                pg_nn.CausalConv2d(True, in_channels=1, out_channels=16, kernel_size=3, padding=1, bias=False)):
        assert not ops.gpt_stem_supported(meta, pos, bad)
    ln, x = pg_nn.NCHWLayerNorm(16), torch.empty(2, 16, 8, 8, device="meta")
    assert ops.gpt_out_head_supported(x, ln, pg_nn.Conv2d(in_channels=16, out_channels=1, kernel_size=1)) == ops.FUSE_ENDS
    assert ops.gpt_out_head_supported(x, ln, pg_nn.Conv2d(in_channels=16, out_channels=4, kernel_size=1)) == ops.FUSE_ENDS
    assert not ops.gpt_out_head_supported(x, ln, pg_nn.Conv2d(in_channels=16, out_channels=5, kernel_size=1))
    assert not ops.gpt_out_head_supported(x, ln, pg_nn.Conv2d(in_channels=16, out_channels=1, kernel_size=1, bias=False))
    assert not ops.gpt_out_head_supported(x, ln, pg_nn.Conv2d(in_channels=16, out_channels=1, kernel_size=3, padding=1))
    assert not ops.gpt_out_head_supported(torch.empty(2, 32, 8, 8, device="meta"), pg_nn.NCHWLayerNorm(32),
                                          pg_nn.Conv2d(in_channels=32, out_channels=1, kernel_size=1))
