"""tsqr_gpu_amd -- MI355X-native tall-skinny QR behind the mtk::qr::qr / mtk::qr::buffer surface.

csrc/      hand-written HIP kernels (gfx950) + the C ABI (include/tsqr_mi.h)
blockqr.py Python mirror of the reference's blockqr.hpp interface (ctypes over the C ABI)
dist.py    row-partitioned multi-GPU TSQR (one process per GPU, R factors all-gathered over RCCL)
"""
from .blockqr import (LstsqRankError, OrthError, QrcpError, SvdError, buffer, buffer_f64_qrcp, buffer_f64_r, buffer_f64_svd, compute_mode,  # noqa: F401
                      error_invalid_matrix_size, error_unsupported_mode, get_batch_size, get_batch_size_log2, get_working_l_size,
                      get_working_q_size, get_working_r_size, last_jacobi_sweeps_f64, lstsq_f64, lstsq_rank_f64, orth_f64, orth_f64_tensor, qr, qr_f64_tensor, qr_f64_wide_tensor,
                      qrcp_f64, qrcp_f64_tensor, r_f64, success_factorization, svd_f64, svd_f64_tensor, tsqr_colmun_size)
