"""torch.autograd bindings of the HIP kernels (the only arithmetic on the hot path).

Every function here launches kernels from libpg_hip.so on torch's *current* HIP stream with
raw device pointers (so a whole training step can be captured into a hipGraph). PyTorch is
used for memory (caching allocator), streams and the autograd tape only.

Weight gradients: if a parameter carries a `_pg_grad` tensor (a view into the trainer's flat
gradient buffer, zeroed once per step) the backward kernels accumulate straight into it with
fp32 atomics and autograd sees `None` for that parameter — no per-parameter AccumulateGrad
kernels, and the flat buffer is what RCCL all-reduces. Without `_pg_grad` the usual
`param.grad` protocol is followed.
"""

# One module per kernel family (round 6: this was a single 1 900-line file); the package re-exports every name, so that
# `from pytorch_generative_amd import ops; ops.conv2d_taps(...)` and the tests' / tools' uses of the helpers are unchanged.
from pytorch_generative_amd.ops._common import (  # noqa: F401
    ACT_NONE,
    ACT_RELU,
    ACT_ELU,
    ACT_GELU,
    ACT_ELU_OUT,
    GATE_TANH,
    GATE_IDENTITY,
    _ACT_IDS,
    _stream,
    RowDecode,
    _chk,
    _p,
    zeros,
    zeros_like,
    _sink,
    _grad_targets,
    CONV_FMT_F32,
    CONV_FMT_B3,
    CONV_FMT_B3_GATE,
    FUSE_SKIP,
    _dense_per_image,
)
from pytorch_generative_amd.ops.elementwise import (  # noqa: F401
    _ConcatChannels,
    concat_channels,
    _Act,
    relu,
    elu,
    gelu,
    _Gated,
    gated_activation,
    _Add,
    add,
    _AddBcast,
    add_broadcast_batch,
    image_positional_encoding,
    mul_inplace_,
    _sum_into,
    _SumVectors,
    _Fanout,
    fanout,
    sum_vectors,
)
from pytorch_generative_amd.ops.conv import (  # noqa: F401
    ConvSpec,
    CONV_MFMA,
    _use_mfma,
    _pack_frag,
    conv_formats,
    _pack,
    _ConvTaps,
    FUSE_PAIR,
    FUSE_LNSKIP,
    FUSE_QKV_EXTRA,
    _adjacent_view,
    conv_pair_views,
    _ConvPair,
    conv2d_pair,
    conv_mfma_ok,
    conv_two_residuals_ok,
    conv2d_taps,
    conv_gate_ok,
    conv_dual_ok,
    GradSlot,
    FUSE_DUAL,
    FUSE_GATE,
)
from pytorch_generative_amd.ops.code_conv import (  # noqa: F401
    CODE_MAX_CODES,
    code_conv2d,
    code_conv_wgrad_plan,
    vq_lookup,
    codes_to_levels,
)
from pytorch_generative_amd.ops.code_up import (  # noqa: F401
    CODE_UP_MAX_FACTOR,
    code_upsample,
    code_upsample_,
    code_up_plan,
    sample_cond_codes_,
)
from pytorch_generative_amd.ops.gpt_block import (  # noqa: F401
    FUSE_MLP,
    mlp_gelu_supported,
    _MlpGelu,
    mlp_gelu,
    FUSE_BLOCK,
    new_block_chain,
    assert_no_pending_block_reductions,
    reduce_rows,
    _GPTBlockHead,
    _GPTBlockTail,
    gpt_block_supported,
    gpt_block_head,
    gpt_block_tail,
    gpt_blocks,
    _NCHWLayerNorm,
    nchw_layernorm,
    nchw_layernorm_skip,
)
from pytorch_generative_amd.ops.gpt_ends import (  # noqa: F401
    FUSE_ENDS,
    gpt_stem_supported,
    _GPTStem,
    gpt_stem,
    gpt_out_head_supported,
    _GPTOutHead,
    gpt_out_head,
)
from pytorch_generative_amd.ops.gpt_decode import (  # noqa: F401
    gpt_decode_plan,
    gpt_decode_supported,
    gpt_decode_pack,
    gpt_decode_step,
)
from pytorch_generative_amd.ops.attention_row import (  # noqa: F401
    attention_row_plan,
    attention_row_supported,
    attention_row,
    row_gather,
)
from pytorch_generative_amd.ops.attention import (  # noqa: F401
    _CausalAttention,
    _CausalAttentionQKV,
    _MergeQKVWeight,
    merge_qkv_weight,
    set_deterministic,
    causal_attention_qkv,
    attention_dims_native,
    attention_route,
    attention_layout_flags,
    _pad16,
    causal_attention,
)
from pytorch_generative_amd.ops.linear_attention import (  # noqa: F401
    _LinearCausalAttention,
    FEATURE_IDENTITY,
    FEATURE_ELU1,
    linear_causal_attention,
)
from pytorch_generative_amd.ops.masked_linear import (  # noqa: F401
    _MaskedMLP,
    mask_from_degrees,
    masked_linear,
    masked_mlp,
    mul_mask_,
)
from pytorch_generative_amd.ops.made_sample import (  # noqa: F401
    made_sample_plan,
    made_sample_chain,
)
from pytorch_generative_amd.ops.nade import (  # noqa: F401
    _NADE,
    nade,
    nade_plan,
)
from pytorch_generative_amd.ops.fvbn import (  # noqa: F401
    _FVBN,
    fvbn,
    fvbn_offsets,
    fvbn_pack,
    fvbn_plan,
    fvbn_plan_status,
    fvbn_sample_chain,
    fvbn_tiles,
    fvbn_unpack,
)
from pytorch_generative_amd.ops.nice import (  # noqa: F401
    _Coupling,
    _NiceScale,
    _LogisticLogProb,
    coupling,
    dense_linear_plan,
    logistic_logprob,
    nice_scale,
)
from pytorch_generative_amd.ops.density import (  # noqa: F401
    _MixtureLogProb,
    MIXTURE_BERNOULLI,
    MIXTURE_GAUSSIAN,
    kde_gaussian,
    kde_parzen,
    mixture_log_prob,
)
from pytorch_generative_amd.ops.linear_categorical import (  # noqa: F401
    DeferredLogits,
    _LinearCategoricalNLL,
    linear_categorical_supported,
)
from pytorch_generative_amd.ops.losses import (  # noqa: F401
    _BCEWithLogitsSumMean,
    _DmolLossSumMean,
    dmol_loss_sum_mean,
    DMOL_SAMPLE_MAX_K,
    dmol_sample,
    bce_with_logits_sum_mean,
    _CategoricalNLLSumMean,
    CATEGORICAL_MAX_CLASSES,
    categorical_nll_sum_mean,
    categorical_nll_per_sample,
    categorical_sample,
    _ElboMean,
    elbo_terms,
)
from pytorch_generative_amd.ops.vae import (  # noqa: F401
    _AvgPool2,
    avg_pool2,
    _Upsample2,
    upsample2_nearest,
    _GaussHead,
    gaussian_head_unit,
    gaussian_head_pair,
    gaussian_head_prior,
    _PhaseSplit,
    _PhaseMerge,
    _PhaseWeights,
    _SplitInChannels,
    split_in_channels,
    phase_weights,
    phase_split,
    phase_merge,
    _PhaseMerge4,
    _PhaseSplit4,
    phase_split4,
    phase_merge4,
    _ConcatElu,
    concat_elu,
    _Resample2,
    subsample2,
    zero_insert2,
    col_subsample2,
    col_zero_insert2,
)
from pytorch_generative_amd.ops.gp import (  # noqa: F401
    GP_PLAN_INTS,
    gp_plan_status,
    gp_plan,
    se_kernel,
    add_diag_,
    gemm_nt_,
    cholesky_,
    trsm_right_,
    GP_MLL_PLAN_INTS,
    gp_mll_plan_status,
    gp_mll_plan,
    tri_inverse_t,
    gram_upper_,
    se_mll_sums,
    mll_value,
    GP_ARD_PLAN_INTS,
    GP_KINDS,
    gp_ard_plan_status,
    gp_ard_plan,
    stationary_kernel,
    stationary_mll_sums,
    ard_mll_sums,
)
