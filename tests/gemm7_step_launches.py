"""The grouped NT / NN launches of one MulT fusion step (B = 16: 8192 text, 6400 audio, 480 video rows; d = 768, FFN 3072) as
generation 7 runs them with the step captured as one chain: (name, layout, flag set, [(M, N, K)], tile width the automatic rule
must give on 256 workgroups)."""
from mmfusion.lib import EPI_ADD_AUX, EPI_BIAS, EPI_MASK_AUX, EPI_RELU, GEMM_NN, GEMM_NT

T, A, V = 8192, 6400, 480
CROSS = (T, T, A, A, V, V)          # each modality is the target of two cross blocks and the source of two
SELF = (T, A, V)

STEP_LAUNCHES = [
    ("fwd in-proj (6 Q + 6 KV)", GEMM_NT, EPI_BIAS, [(m, 768, 768) for m in CROSS] + [(m, 1536, 768) for m in CROSS], 192),
    ("fwd out-proj + residual", GEMM_NT, EPI_BIAS | EPI_ADD_AUX, [(m, 768, 768) for m in CROSS], 192),
    ("fwd ffn1", GEMM_NT, EPI_BIAS | EPI_RELU, [(m, 3072, 768) for m in CROSS], 256),
    ("fwd ffn2 + residual", GEMM_NT, EPI_BIAS | EPI_ADD_AUX, [(m, 768, 3072) for m in CROSS], 192),
    ("fwd self QKV", GEMM_NT, EPI_BIAS, [(m, 2304, 768) for m in SELF], 192),
    ("bwd self-QKV dgrad", GEMM_NN, 0, [(m, 768, 2304) for m in SELF], 192),
    ("bwd ffn2 dgrad dH", GEMM_NN, EPI_MASK_AUX, [(m, 3072, 768) for m in CROSS], 256),
    ("bwd ffn1 dgrad dX", GEMM_NN, EPI_ADD_AUX, [(m, 768, 3072) for m in CROSS], 192),
    ("bwd out-proj dgrad", GEMM_NN, 0, [(m, 768, 768) for m in CROSS], 192),
    ("bwd in-proj dgrad", GEMM_NN, 0, [(m, 768, 768) for m in CROSS] + [(m, 768, 1536) for m in CROSS], 192),
]
