// The argument checks of the C entry points (rjprt.hip) that are pure functions of the caller's
// structs: no HIP call, nothing but include/rjprt.h and the standard library, so that a plain C++
// program can feed them hand-built structs (tests/test_host_logic.py).  Each returns RJP_OK or the
// status of the refusal and writes its message to `err`; rjprt.hip hands both to fail().  The
// messages are part of the library's behaviour (tests/golden/abi_refusals.json).  Limits that
// live with the kernels (RJP_SGPR_BURSTS, RJP_LT_MAX_K, RJP_SRT_MAX_K) are passed in.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rjprt.h"

namespace rjp_args {

inline bool mode_ok(int m) { return m == RJP_GFF_SCALAR || m == RJP_GFF_POWERLAW; }

inline int refuse(std::string& err, const std::string& what, int code = RJP_ERR_ARG) {
  err = what;
  return code;
}

inline int check_y_pair(const rjp_fields* f, std::string& err) {
  if ((f->d_ylo == nullptr) != (f->d_yhi == nullptr))
    return refuse(err, "fields.d_ylo and d_yhi must both be set or both be NULL");
  return RJP_OK;
}

// storage tag and dimensions of a non-NULL rjp_fields; `y_pair`: and the d_ylo / d_yhi pairing
inline int check_grid(const rjp_fields* f, bool y_pair, std::string& err) {
  if (f->dtype != RJP_F32 && f->dtype != RJP_F64)
    return refuse(err, "fields.dtype must be RJP_F32 (4) or RJP_F64 (8)");
  if (f->nx <= 0 || f->ny <= 0 || f->nz <= 0)
    return refuse(err, "grid dimensions must be positive");
  return y_pair ? check_y_pair(f, err) : RJP_OK;
}

// `compact_ok`: the entry point can run from the compact layout alone (d_em0 + d_temp);
// `tau_mode` >= 0: ... or from the tau layout alone (d_a0 built for that mode)
inline int check_fields(const rjp_fields* f, bool need_vy, bool compact_ok, int tau_mode,
                        std::string& err) {
  if (!f) return refuse(err, "fields is NULL");
  if (int r = check_grid(f, false, err)) return r;
  if (f->d_a0 && (f->dtype != RJP_F64 || !mode_ok(f->a0_mode)))
    return refuse(err, "fields.d_a0 needs RJP_F64 storage and a valid a0_mode");
  if (tau_mode >= 0 && f->d_a0 && f->a0_mode == tau_mode) {
    // nothing else is needed for the scan itself (d_em0 / d_temp are checked where asked for)
  } else if (compact_ok && f->d_em0) {
    if (!f->d_temp) return refuse(err, "fields.d_temp must be a device pointer");
  } else if (!f->d_nd || !f->d_xi || !f->d_temp || !f->d_pf) {
    return refuse(err, "fields nd/xi/temp/pf must be device pointers");
  }
  if (need_vy && !f->d_vy) return refuse(err, "fields.d_vy required for RRL");
  if (!(f->csize_au > 0.0)) return refuse(err, "fields.csize_au must be > 0");
  return check_y_pair(f, err);
}

// (`f` non-NULL: after check_fields)
inline int check_bursts(const rjp_bursts* b, const rjp_fields* f, std::string& err) {
  if (!b) return RJP_OK;
  for (int j = 0; j < 2; ++j) {
    if (b->n[j] < 0 || b->n[j] > (1 << 20)) return refuse(err, "bursts.n must be >= 0");
    if (b->n[j] > 0 && (!b->t0[j] || !b->amp_rel[j] || !b->inv2s2[j]))
      return refuse(err, "bursts: NULL parameter array for a jet with n > 0");
    if (b->n[j] > 0 && !f->d_ts)
      return refuse(err, "fields.d_ts required when bursts are present");
  }
  return RJP_OK;
}

// the epoch list of a sweep; `finite`: every epoch must be a finite number
inline int check_epochs(const double* epochs, int n_epochs, bool finite, const char* who,
                        std::string& err) {
  if (!epochs || n_epochs < 1)
    return refuse(err, std::string(who) + ": NULL epochs or n_epochs < 1");
  for (int e = 0; finite && e < n_epochs; ++e)
    if (!std::isfinite(epochs[e])) return refuse(err, std::string(who) + ": non-finite epoch");
  return RJP_OK;
}

// The bursts a sensitivity call differentiates with respect to, and its epochs, in the order the
// entry points refuse them: no burst, check_bursts, more than `max_bursts` in a jet, the epochs,
// a non-finite burst parameter.  Fills the chain-rule table -- per burst (2 amp inv2s2, 1, -amp)
// for (t0, amp_rel, inv2s2), behind a leading 1 with `lead` -- into `scale`, which holds
// lead + 6 * max_bursts doubles, and returns its length in `n_scale`.
inline int check_grad_bursts(const rjp_bursts* b, const rjp_fields* f, const double* epochs,
                             int n_epochs, int max_bursts, bool lead, const char* who,
                             double* scale, int* n_scale, std::string& err) {
  const std::string w(who);
  if (!b || b->n[0] + b->n[1] <= 0 || b->n[0] < 0 || b->n[1] < 0)
    return refuse(err, w + ": no burst to differentiate with respect to");
  if (int r = check_bursts(b, f, err)) return r;
  if (b->n[0] > max_bursts || b->n[1] > max_bursts)
    return refuse(err, w + ": more than " + std::to_string(max_bursts) + " bursts in a jet");
  if (int r = check_epochs(epochs, n_epochs, true, who, err)) return r;
  int k = 0;
  if (lead) scale[k++] = 1.0;
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < b->n[j]; ++i, k += 3) {
      const double t0 = b->t0[j][i], amp = b->amp_rel[j][i], inv = b->inv2s2[j][i];
      if (!std::isfinite(t0) || !std::isfinite(amp) || !std::isfinite(inv))
        return refuse(err, w + ": non-finite burst parameter");
      scale[k] = 2.0 * amp * inv;
      scale[k + 1] = 1.0;
      scale[k + 2] = -amp;
    }
  *n_scale = k;
  return RJP_OK;
}

// What a launch-time layout (`name`: "launch-time-ordered layout", ...) is built from: f64 fields
// with d_a0 and d_ts, 1 <= K <= max_K bins per jet, the launch-time range; `max_ny` > 0: n_y
// below it
inline int check_layout(const rjp_fields* f, int K, const char* name, int max_K, int max_ny,
                        std::string& err) {
  const std::string w(name);
  if (!f) return refuse(err, "fields is NULL");
  if (f->dtype != RJP_F64 || !f->d_a0 || !f->d_ts)
    return refuse(err, w + ": needs RJP_F64 fields with d_a0 and d_ts");
  if (f->nx <= 0 || f->ny <= 0 || f->nz <= 0 || (max_ny > 0 && f->ny >= max_ny))
    return refuse(err, w + ": grid dimensions must be positive" +
                           (max_ny > 0 ? ", n_y < " + std::to_string(max_ny) : std::string()));
  if (K < 1 || K > max_K) return refuse(err, w + ": 1 <= K <= " + std::to_string(max_K));
  if (!(f->ts_hi >= f->ts_lo) || !std::isfinite(f->ts_lo) || !std::isfinite(f->ts_hi) ||
      (f->ts_lo == 0.0 && f->ts_hi == 0.0))
    return refuse(err, w + ": fields.ts_lo / ts_hi (rjp_field_range) required");
  return RJP_OK;
}

// What rjp_srt_codes takes, in the order it refuses: check_layout's refusals (NULL fields, storage,
// dimensions, K, no launch-time range), a NULL pointer, a pointer read or written in 16-byte units
// that is not 16-byte aligned.
inline int check_srt_codes(const rjp_fields* f, int K, int max_K, const void* d_start,
                           const void* d_rowbase, const void* d_cells, const void* d_pc,
                           std::string& err) {
  if (int r = check_layout(f, K, "launch-time-bucketed layout", max_K, 0, err)) return r;
  if (!d_start || !d_rowbase || !d_cells || !d_pc)
    return refuse(err, "rjp_srt_codes: NULL argument");
  if (((uintptr_t)d_cells % 16) != 0 || ((uintptr_t)d_pc % 16) != 0)
    return refuse(err, "rjp_srt_codes: d_cells and d_pc must be 16-byte aligned");
  return RJP_OK;
}

// What rjp_vis_adjoint takes, in the order it refuses: NULL pointers, counts below 1, a non-finite
// scale.  (`d_w` may be NULL; the grid and the workspace are checked where the tiling lives.)
inline int check_vis_adjoint(const double* d_vis, int n_maps, int n_vis, const double* h_su,
                             const double* h_sv, const double* d_u, const double* d_v, int nx,
                             int nz, const double* d_img, std::string& err) {
  if (!d_vis || !h_su || !h_sv || !d_u || !d_v || !d_img)
    return refuse(err, "rjp_vis_adjoint: NULL visibilities, scales, baselines or output");
  if (n_maps < 1 || n_vis < 1 || nx < 1 || nz < 1)
    return refuse(err, "rjp_vis_adjoint: n_maps, n_vis, nx and nz must be positive");
  for (int m = 0; m < n_maps; ++m)
    if (!std::isfinite(h_su[m]) || !std::isfinite(h_sv[m]))
      return refuse(err, "rjp_vis_adjoint: non-finite h_su / h_sv");
  return RJP_OK;
}

// What rjp_clean takes, in the order it refuses: NULL pointers, sizes below 1, an even beam, the
// beam count, the image size, the gain, n_iter, the thresholds.  (`d_mask`, `d_model`, `d_peak`
// may be NULL; the grid and the workspace are checked where the tiling lives.)
inline int check_clean(const double* d_res, int n_maps, int nx, int nz, const double* d_psf,
                       int n_psf, int px, int pz, const double* h_thresh, double gain, int n_iter,
                       const int32_t* d_cpix, const double* d_cflux, const int32_t* d_ncomp,
                       std::string& err) {
  if (!d_res || !d_psf || !h_thresh || !d_cpix || !d_cflux || !d_ncomp)
    return refuse(err, "rjp_clean: NULL images, beams, thresholds or component outputs");
  if (n_maps < 1 || nx < 1 || nz < 1 || px < 1 || pz < 1)
    return refuse(err, "rjp_clean: n_maps, nx, nz, px and pz must be positive");
  if (px % 2 == 0 || pz % 2 == 0)
    return refuse(err, "rjp_clean: px and pz must be odd (the beam's centre is a pixel)");
  if (n_psf != 1 && n_psf != n_maps)
    return refuse(err, "rjp_clean: n_psf must be 1 or n_maps");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_clean: nx * nz exceeds 2^31 - 1");
  if (!(gain > 0.0 && gain <= 1.0)) return refuse(err, "rjp_clean: gain must lie in (0, 1]");
  if (n_iter < 1) return refuse(err, "rjp_clean: n_iter < 1");
  for (int m = 0; m < n_maps; ++m)
    if (!(h_thresh[m] >= 0.0) || !std::isfinite(h_thresh[m]))
      return refuse(err, "rjp_clean: negative or non-finite threshold");
  return RJP_OK;
}

// What rjp_convolve2d takes, in the order it refuses: NULL pointers, sizes below 1, an even kernel
// size, a kernel beyond RJP_CONV_MAX_K, the kernel count, the image size, the workgroup count of
// the tile rule (RJP_CONV_TILE_X x RJP_CONV_TILE_Z output pixels).  (`d_add` may be NULL.)
inline int check_convolve2d(const double* d_in, int n_maps, int nx, int nz, const double* d_ker,
                            int n_ker, int kx, int kz, const double* d_out, std::string& err) {
  if (!d_in || !d_ker || !d_out) return refuse(err, "rjp_convolve2d: NULL input, kernels or output");
  if (n_maps < 1 || nx < 1 || nz < 1 || kx < 1 || kz < 1)
    return refuse(err, "rjp_convolve2d: n_maps, nx, nz, kx and kz must be positive");
  if (kx % 2 == 0 || kz % 2 == 0)
    return refuse(err, "rjp_convolve2d: kx and kz must be odd (the kernel's centre is a pixel)");
  if (kx > RJP_CONV_MAX_K || kz > RJP_CONV_MAX_K)
    return refuse(err, "rjp_convolve2d: kx and kz must not exceed RJP_CONV_MAX_K (" +
                           std::to_string(RJP_CONV_MAX_K) + ")");
  if (n_ker != 1 && n_ker != n_maps)
    return refuse(err, "rjp_convolve2d: n_ker must be 1 or n_maps");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_convolve2d: nx * nz exceeds 2^31 - 1");
  const int64_t tiles = (((int64_t)nx + RJP_CONV_TILE_X - 1) / RJP_CONV_TILE_X) *
                        (((int64_t)nz + RJP_CONV_TILE_Z - 1) / RJP_CONV_TILE_Z);
  if (tiles > (int64_t)INT32_MAX / n_maps)
    return refuse(err, "rjp_convolve2d: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_msclean takes, in the order it refuses: NULL pointers, sizes below 1, an even beam, the
// beam count, the image size, the gain, n_iter, the thresholds, the weights.  (`d_mask`, `d_model`,
// `d_peak` may be NULL; the grid and the workspace are checked where the tiling lives.)
inline int check_msclean(const double* d_res, int n_maps, int n_s, int nx, int nz,
                         const double* d_xpsf, int n_psf, int px, int pz, const double* h_weight,
                         const double* h_thresh, double gain, int n_iter, const int32_t* d_cpix,
                         const int32_t* d_cscale, const double* d_cflux, const int32_t* d_ncomp,
                         std::string& err) {
  if (!d_res || !d_xpsf || !h_weight || !h_thresh || !d_cpix || !d_cscale || !d_cflux || !d_ncomp)
    return refuse(err, "rjp_msclean: NULL planes, cross beams, weights, thresholds or component "
                       "outputs");
  if (n_maps < 1 || n_s < 1 || nx < 1 || nz < 1 || px < 1 || pz < 1)
    return refuse(err, "rjp_msclean: n_maps, n_s, nx, nz, px and pz must be positive");
  if (px % 2 == 0 || pz % 2 == 0)
    return refuse(err, "rjp_msclean: px and pz must be odd (the beam's centre is a pixel)");
  if (n_psf != 1 && n_psf != n_maps)
    return refuse(err, "rjp_msclean: n_psf must be 1 or n_maps");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_msclean: nx * nz exceeds 2^31 - 1");
  if (!(gain > 0.0 && gain <= 1.0)) return refuse(err, "rjp_msclean: gain must lie in (0, 1]");
  if (n_iter < 1) return refuse(err, "rjp_msclean: n_iter < 1");
  for (int m = 0; m < n_maps; ++m)
    if (!(h_thresh[m] >= 0.0) || !std::isfinite(h_thresh[m]))
      return refuse(err, "rjp_msclean: negative or non-finite threshold");
  for (int64_t i = 0; i < (int64_t)n_maps * n_s; ++i)
    if (!(h_weight[i] >= 0.0) || !std::isfinite(h_weight[i]))
      return refuse(err, "rjp_msclean: negative or non-finite weight");
  return RJP_OK;
}

// What rjp_mtmfs takes, in the order it refuses: NULL pointers, sizes below 1, n_t beyond
// RJP_MTMFS_MAX_NT, an even beam, the beam count, the image size, the gain, n_iter, the thresholds,
// the inverse Hessians.  (`d_mask`, `d_model`, `d_peak` may be NULL; the grid and the workspace are
// checked where the tiling lives.)
inline int check_mtmfs(const double* d_res, int n_maps, int n_t, int nx, int nz,
                       const double* d_spsf, int n_psf, int px, int pz, const double* h_hinv,
                       const double* h_thresh, double gain, int n_iter, const int32_t* d_cpix,
                       const double* d_ccoef, const int32_t* d_ncomp, std::string& err) {
  if (!d_res || !d_spsf || !h_hinv || !h_thresh || !d_cpix || !d_ccoef || !d_ncomp)
    return refuse(err, "rjp_mtmfs: NULL planes, spectral beams, inverse Hessians, thresholds or "
                       "component outputs");
  if (n_maps < 1 || n_t < 1 || nx < 1 || nz < 1 || px < 1 || pz < 1)
    return refuse(err, "rjp_mtmfs: n_maps, n_t, nx, nz, px and pz must be positive");
  if (n_t > RJP_MTMFS_MAX_NT)
    return refuse(err, "rjp_mtmfs: n_t must not exceed RJP_MTMFS_MAX_NT (" +
                           std::to_string(RJP_MTMFS_MAX_NT) + ")");
  if (px % 2 == 0 || pz % 2 == 0)
    return refuse(err, "rjp_mtmfs: px and pz must be odd (the beam's centre is a pixel)");
  if (n_psf != 1 && n_psf != n_maps)
    return refuse(err, "rjp_mtmfs: n_psf must be 1 or n_maps");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_mtmfs: nx * nz exceeds 2^31 - 1");
  if (!(gain > 0.0 && gain <= 1.0)) return refuse(err, "rjp_mtmfs: gain must lie in (0, 1]");
  if (n_iter < 1) return refuse(err, "rjp_mtmfs: n_iter < 1");
  for (int m = 0; m < n_maps; ++m)
    if (!(h_thresh[m] >= 0.0) || !std::isfinite(h_thresh[m]))
      return refuse(err, "rjp_mtmfs: negative or non-finite threshold");
  for (int64_t i = 0; i < (int64_t)n_maps * n_t * n_t; ++i)
    if (!std::isfinite(h_hinv[i])) return refuse(err, "rjp_mtmfs: non-finite h_hinv");
  return RJP_OK;
}

// What rjp_vis_components takes, in the order it refuses: NULL pointers, sizes below 1, the sign, a
// missing d_gvis with more than one scale, a non-finite scale, the image size, the workgroup count
// (64 visibilities each).  (`d_cscale`, `d_gvis` and `d_in` may be NULL.)
inline int check_vis_components(const int32_t* d_cpix, const double* d_cflux,
                                const int32_t* d_ncomp, int n_maps, int comp_stride, int n_s, int nx,
                                int nz, const double* h_su, const double* h_sv, const double* d_u,
                                const double* d_v, int n_vis, const double* d_gvis, int sign,
                                const double* d_out, std::string& err) {
  if (!d_cpix || !d_cflux || !d_ncomp || !h_su || !h_sv || !d_u || !d_v || !d_out)
    return refuse(err, "rjp_vis_components: NULL components, scales, baselines or output");
  if (n_maps < 1 || comp_stride < 1 || n_s < 1 || nx < 1 || nz < 1 || n_vis < 1)
    return refuse(err, "rjp_vis_components: n_maps, comp_stride, n_s, nx, nz and n_vis must be "
                       "positive");
  if (sign != 1 && sign != -1) return refuse(err, "rjp_vis_components: sign must be +1 or -1");
  if (!d_gvis && n_s != 1)
    return refuse(err, "rjp_vis_components: a NULL d_gvis (G = 1) needs n_s = 1");
  for (int m = 0; m < n_maps; ++m)
    if (!std::isfinite(h_su[m]) || !std::isfinite(h_sv[m]))
      return refuse(err, "rjp_vis_components: non-finite h_su / h_sv");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_vis_components: nx * nz exceeds 2^31 - 1");
  if (((int64_t)n_vis + 63) / 64 > (int64_t)INT32_MAX / n_maps)
    return refuse(err, "rjp_vis_components: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_components_image takes, in the order it refuses: NULL pointers, sizes below 1, the image
// size, the workgroup count (256 pixels of one plane each).  (`d_cscale` may be NULL.)
inline int check_components_image(const int32_t* d_cpix, const double* d_cflux,
                                  const int32_t* d_ncomp, int n_maps, int comp_stride, int n_s,
                                  int nx, int nz, const double* d_out, std::string& err) {
  if (!d_cpix || !d_cflux || !d_ncomp || !d_out)
    return refuse(err, "rjp_components_image: NULL components or output");
  if (n_maps < 1 || comp_stride < 1 || n_s < 1 || nx < 1 || nz < 1)
    return refuse(err, "rjp_components_image: n_maps, comp_stride, n_s, nx and nz must be positive");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_components_image: nx * nz exceeds 2^31 - 1");
  if ((((int64_t)nx * nz + 255) / 256) * n_s > (int64_t)INT32_MAX / n_maps)
    return refuse(err, "rjp_components_image: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_restore takes, in the order it refuses: NULL pointers, sizes below 1, the image size, a
// beam whose quadratic form is not positive definite (or not finite).  (`d_add` may be NULL.)
inline int check_restore(const int32_t* d_cpix, const double* d_cflux, const int32_t* d_ncomp,
                         int n_maps, int comp_stride, const double* h_beam, int nx, int nz,
                         const double* d_out, std::string& err) {
  if (!d_cpix || !d_cflux || !d_ncomp || !h_beam || !d_out)
    return refuse(err, "rjp_restore: NULL components, beams or output");
  if (n_maps < 1 || comp_stride < 1 || nx < 1 || nz < 1)
    return refuse(err, "rjp_restore: n_maps, comp_stride, nx and nz must be positive");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_restore: nx * nz exceeds 2^31 - 1");
  for (int m = 0; m < n_maps; ++m) {
    const double A = h_beam[3 * m], B = h_beam[3 * m + 1], C = h_beam[3 * m + 2];
    if (!std::isfinite(A) || !std::isfinite(B) || !std::isfinite(C) || !(A > 0.0) || !(C > 0.0) ||
        !(A * C > B * B))
      return refuse(err, "rjp_restore: the beam (A, B, C) must be positive definite");
  }
  return RJP_OK;
}

// What rjp_gaussfit takes, in the order it refuses: NULL pointers, sizes below 1, the image size,
// the box, lambda0 and xtol, n_iter.  (`d_mask` and `d_trace` may be NULL; the grid and the workspace
// are checked where the tiling lives.)
inline int check_gaussfit(const double* d_img, int n_maps, int nx, int nz, const int32_t* h_box,
                          const double* d_theta, double lambda0, double xtol, int n_iter,
                          const double* d_chi2, const double* d_cov, const int32_t* d_npix,
                          const int32_t* d_niter, const int32_t* d_status, std::string& err) {
  if (!d_img || !h_box || !d_theta || !d_chi2 || !d_cov || !d_npix || !d_niter || !d_status)
    return refuse(err, "rjp_gaussfit: NULL images, box, parameters or outputs");
  if (n_maps < 1 || nx < 1 || nz < 1)
    return refuse(err, "rjp_gaussfit: n_maps, nx and nz must be positive");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX)
    return refuse(err, "rjp_gaussfit: nx * nz exceeds 2^31 - 1");
  if (h_box[0] < 0 || h_box[1] >= nx || h_box[1] < h_box[0] || h_box[2] < 0 || h_box[3] >= nz ||
      h_box[3] < h_box[2])
    return refuse(err, "rjp_gaussfit: the box (i0, i1, j0, j1) must lie inside the image, "
                       "i0 <= i1 and j0 <= j1");
  if (!(lambda0 > 0.0) || !std::isfinite(lambda0) || !(xtol > 0.0) || !std::isfinite(xtol))
    return refuse(err, "rjp_gaussfit: lambda0 and xtol must be finite and positive");
  if (n_iter < 1) return refuse(err, "rjp_gaussfit: n_iter < 1");
  return RJP_OK;
}

// What rjp_uvfit takes, in the order it refuses: NULL pointers, counts below 1, n_comp, w_maps, a
// non-finite scale, no free parameter, lambda0 and xtol, n_iter, the workgroup count (1024
// visibilities each).  (`d_w`, `h_free` and `d_trace` may be NULL; the workspace is checked where
// the tiling lives.)
inline int check_uvfit(const double* d_vis, int n_maps, int n_vis, const double* h_su,
                       const double* h_sv, const double* d_u, const double* d_v, const double* d_w,
                       int w_maps, int n_comp, const uint8_t* h_free, const double* d_theta,
                       double lambda0, double xtol, int n_iter, const double* d_chi2,
                       const double* d_cov, const int32_t* d_nvis, const int32_t* d_niter,
                       const int32_t* d_status, std::string& err) {
  if (!d_vis || !h_su || !h_sv || !d_u || !d_v || !d_theta || !d_chi2 || !d_cov || !d_nvis ||
      !d_niter || !d_status)
    return refuse(err, "rjp_uvfit: NULL visibilities, scales, baselines, parameters or outputs");
  if (n_maps < 1 || n_vis < 1) return refuse(err, "rjp_uvfit: n_maps and n_vis must be positive");
  if (n_comp < 1 || n_comp > RJP_UVFIT_MAX_COMP)
    return refuse(err, "rjp_uvfit: n_comp must lie in 1 .. RJP_UVFIT_MAX_COMP (" +
                           std::to_string(RJP_UVFIT_MAX_COMP) + ")");
  if (d_w && w_maps != 1 && w_maps != n_maps)
    return refuse(err, "rjp_uvfit: w_maps must be 1 or n_maps");
  for (int m = 0; m < n_maps; ++m)
    if (!std::isfinite(h_su[m]) || !std::isfinite(h_sv[m]))
      return refuse(err, "rjp_uvfit: non-finite h_su / h_sv");
  if (h_free) {
    bool any = false;
    for (int i = 0; i < 6 * n_comp; ++i) any = any || h_free[i] != 0;
    if (!any) return refuse(err, "rjp_uvfit: no free parameter");
  }
  if (!(lambda0 > 0.0) || !std::isfinite(lambda0) || !(xtol > 0.0) || !std::isfinite(xtol))
    return refuse(err, "rjp_uvfit: lambda0 and xtol must be finite and positive");
  if (n_iter < 1) return refuse(err, "rjp_uvfit: n_iter < 1");
  if (((int64_t)n_vis + 1023) / 1024 > (int64_t)INT32_MAX / n_maps)
    return refuse(err, "rjp_uvfit: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_cube_moments takes, in the order it refuses: NULL pointers, sizes below 1, the channel
// limit, the axis, the widths, x_ref, clip, the workgroup count (64 pixels each).  (`d_mask`,
// `d_ipeak` and `d_count` may be NULL.)
inline int check_cube_moments(const double* d_cube, int64_t n_pix, int n_chan, const double* h_x,
                              const double* h_dx, double x_ref, double clip, const double* d_mom,
                              std::string& err) {
  if (!d_cube || !h_x || !h_dx || !d_mom)
    return refuse(err, "rjp_cube_moments: NULL cube, axis, widths or output");
  if (n_pix < 1 || n_chan < 1)
    return refuse(err, "rjp_cube_moments: n_pix and n_chan must be positive");
  if (n_chan > RJP_SPECFIT_MAX_CHAN)
    return refuse(err, "rjp_cube_moments: n_chan exceeds RJP_SPECFIT_MAX_CHAN (" +
                           std::to_string(RJP_SPECFIT_MAX_CHAN) + ")");
  for (int c = 0; c < n_chan; ++c)
    if (!std::isfinite(h_x[c])) return refuse(err, "rjp_cube_moments: non-finite h_x");
  for (int c = 0; c < n_chan; ++c)
    if (!(h_dx[c] >= 0.0) || !std::isfinite(h_dx[c]))
      return refuse(err, "rjp_cube_moments: negative or non-finite h_dx");
  if (!std::isfinite(x_ref)) return refuse(err, "rjp_cube_moments: non-finite x_ref");
  if (!(clip >= 0.0) || !std::isfinite(clip))
    return refuse(err, "rjp_cube_moments: clip must be finite and >= 0");
  if ((n_pix + 63) / 64 > (int64_t)INT32_MAX)
    return refuse(err, "rjp_cube_moments: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_specfit takes, in the order it refuses: NULL pointers, sizes below 1, the channel limit,
// n_comp, the axis, x_ref, the weights, no free parameter, lambda0 and xtol, n_iter, the workgroup
// count (64 pixels each).  (`h_w`, `h_free`, `d_mask` and `d_trace` may be NULL.)
inline int check_specfit(const double* d_cube, int64_t n_pix, int n_chan, const double* h_x,
                         double x_ref, const double* h_w, int n_comp, const uint8_t* h_free,
                         const double* d_theta, double lambda0, double xtol, int n_iter,
                         const double* d_chi2, const double* d_cov, const int32_t* d_nchan,
                         const int32_t* d_niter, const int32_t* d_status, std::string& err) {
  if (!d_cube || !h_x || !d_theta || !d_chi2 || !d_cov || !d_nchan || !d_niter || !d_status)
    return refuse(err, "rjp_specfit: NULL cube, axis, parameters or outputs");
  if (n_pix < 1 || n_chan < 1) return refuse(err, "rjp_specfit: n_pix and n_chan must be positive");
  if (n_chan > RJP_SPECFIT_MAX_CHAN)
    return refuse(err, "rjp_specfit: n_chan exceeds RJP_SPECFIT_MAX_CHAN (" +
                           std::to_string(RJP_SPECFIT_MAX_CHAN) + ")");
  if (n_comp < 1 || n_comp > RJP_SPECFIT_MAX_COMP)
    return refuse(err, "rjp_specfit: n_comp must lie in 1 .. RJP_SPECFIT_MAX_COMP (" +
                           std::to_string(RJP_SPECFIT_MAX_COMP) + ")");
  for (int c = 0; c < n_chan; ++c)
    if (!std::isfinite(h_x[c])) return refuse(err, "rjp_specfit: non-finite h_x");
  if (!std::isfinite(x_ref)) return refuse(err, "rjp_specfit: non-finite x_ref");
  if (h_w)
    for (int c = 0; c < n_chan; ++c)
      if (!(h_w[c] >= 0.0) || !std::isfinite(h_w[c]))
        return refuse(err, "rjp_specfit: negative or non-finite h_w");
  if (h_free) {
    bool any = false;
    for (int i = 0; i < 3 * n_comp + 2; ++i) any = any || h_free[i] != 0;
    if (!any) return refuse(err, "rjp_specfit: no free parameter");
  }
  if (!(lambda0 > 0.0) || !std::isfinite(lambda0) || !(xtol > 0.0) || !std::isfinite(xtol))
    return refuse(err, "rjp_specfit: lambda0 and xtol must be finite and positive");
  if (n_iter < 1) return refuse(err, "rjp_specfit: n_iter < 1");
  if ((n_pix + 63) / 64 > (int64_t)INT32_MAX)
    return refuse(err, "rjp_specfit: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_voigtfit takes: rjp_specfit's list in rjp_specfit's order, with 4 n_comp + 2 parameters.
inline int check_voigtfit(const double* d_cube, int64_t n_pix, int n_chan, const double* h_x,
                          double x_ref, const double* h_w, int n_comp, const uint8_t* h_free,
                          const double* d_theta, double lambda0, double xtol, int n_iter,
                          const double* d_chi2, const double* d_cov, const int32_t* d_nchan,
                          const int32_t* d_niter, const int32_t* d_status, std::string& err) {
  if (!d_cube || !h_x || !d_theta || !d_chi2 || !d_cov || !d_nchan || !d_niter || !d_status)
    return refuse(err, "rjp_voigtfit: NULL cube, axis, parameters or outputs");
  if (n_pix < 1 || n_chan < 1) return refuse(err, "rjp_voigtfit: n_pix and n_chan must be positive");
  if (n_chan > RJP_SPECFIT_MAX_CHAN)
    return refuse(err, "rjp_voigtfit: n_chan exceeds RJP_SPECFIT_MAX_CHAN (" +
                           std::to_string(RJP_SPECFIT_MAX_CHAN) + ")");
  if (n_comp < 1 || n_comp > RJP_VOIGTFIT_MAX_COMP)
    return refuse(err, "rjp_voigtfit: n_comp must lie in 1 .. RJP_VOIGTFIT_MAX_COMP (" +
                           std::to_string(RJP_VOIGTFIT_MAX_COMP) + ")");
  for (int c = 0; c < n_chan; ++c)
    if (!std::isfinite(h_x[c])) return refuse(err, "rjp_voigtfit: non-finite h_x");
  if (!std::isfinite(x_ref)) return refuse(err, "rjp_voigtfit: non-finite x_ref");
  if (h_w)
    for (int c = 0; c < n_chan; ++c)
      if (!(h_w[c] >= 0.0) || !std::isfinite(h_w[c]))
        return refuse(err, "rjp_voigtfit: negative or non-finite h_w");
  if (h_free) {
    bool any = false;
    for (int i = 0; i < 4 * n_comp + 2; ++i) any = any || h_free[i] != 0;
    if (!any) return refuse(err, "rjp_voigtfit: no free parameter");
  }
  if (!(lambda0 > 0.0) || !std::isfinite(lambda0) || !(xtol > 0.0) || !std::isfinite(xtol))
    return refuse(err, "rjp_voigtfit: lambda0 and xtol must be finite and positive");
  if (n_iter < 1) return refuse(err, "rjp_voigtfit: n_iter < 1");
  if ((n_pix + 63) / 64 > (int64_t)INT32_MAX)
    return refuse(err, "rjp_voigtfit: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// The interval table of K22: h_sol[0] = 0, steps of 0 or 1, n_sol = h_sol[n_t - 1] + 1.
inline bool sol_ok(const int32_t* h_sol, int n_t, int n_sol) {
  if (h_sol[0] != 0) return false;
  for (int t = 1; t < n_t; ++t)
    if (h_sol[t] != h_sol[t - 1] && h_sol[t] != h_sol[t - 1] + 1) return false;
  return h_sol[n_t - 1] + 1 == n_sol;
}

// What rjp_gain_apply takes, in the order it refuses: NULL pointers, counts below 1, n_ant, the
// interval table, g_maps, the mode, the workgroup count (256 visibilities each).
inline int check_gain_apply(const double* d_vis, int n_maps, int n_t, int n_ant,
                            const double* d_gains, int g_maps, const int32_t* h_sol, int n_sol,
                            int mode, const double* d_out, std::string& err) {
  if (!d_vis || !d_gains || !h_sol || !d_out)
    return refuse(err, "rjp_gain_apply: NULL visibilities, gains, intervals or output");
  if (n_maps < 1 || n_t < 1 || n_sol < 1)
    return refuse(err, "rjp_gain_apply: n_maps, n_t and n_sol must be positive");
  if (n_ant < 2 || n_ant > RJP_GAINCAL_MAX_ANT)
    return refuse(err, "rjp_gain_apply: n_ant must lie in 2 .. RJP_GAINCAL_MAX_ANT (" +
                           std::to_string(RJP_GAINCAL_MAX_ANT) + ")");
  if (!sol_ok(h_sol, n_t, n_sol))
    return refuse(err, "rjp_gain_apply: h_sol must start at 0, rise in steps of 0 or 1 and end at "
                       "n_sol - 1");
  if (g_maps != 1 && g_maps != n_maps)
    return refuse(err, "rjp_gain_apply: g_maps must be 1 or n_maps");
  if (mode != 0 && mode != 1)
    return refuse(err, "rjp_gain_apply: mode must be 0 (corrupt) or 1 (correct)");
  const int64_t n_bl = (int64_t)n_ant * (n_ant - 1) / 2;
  if (((int64_t)n_maps * n_t * n_bl + 255) / 256 > (int64_t)INT32_MAX)
    return refuse(err, "rjp_gain_apply: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_gaincal takes, in the order it refuses: NULL pointers, counts below 1, n_ant, the
// interval table, model_maps and w_maps, the mode, refant, min_bl, tol, n_iter, the workgroup
// count.  (`d_w` and `d_trace` may be NULL; the workspace is checked where its size lives.)
inline int check_gaincal(const double* d_vis, int n_maps, int n_t, int n_ant,
                         const double* d_model, int model_maps, const double* d_w, int w_maps,
                         const int32_t* h_sol, int n_sol, int mode, int refant, int min_bl,
                         double tol, int n_iter, const double* d_gains, const double* d_chi2,
                         const int32_t* d_nvis, const int32_t* d_niter, const int32_t* d_status,
                         const uint8_t* d_live, std::string& err) {
  if (!d_vis || !d_model || !h_sol || !d_gains || !d_chi2 || !d_nvis || !d_niter || !d_status ||
      !d_live)
    return refuse(err, "rjp_gaincal: NULL visibilities, model, intervals, gains or outputs");
  if (n_maps < 1 || n_t < 1 || n_sol < 1)
    return refuse(err, "rjp_gaincal: n_maps, n_t and n_sol must be positive");
  if (n_ant < 2 || n_ant > RJP_GAINCAL_MAX_ANT)
    return refuse(err, "rjp_gaincal: n_ant must lie in 2 .. RJP_GAINCAL_MAX_ANT (" +
                           std::to_string(RJP_GAINCAL_MAX_ANT) + ")");
  if (!sol_ok(h_sol, n_t, n_sol))
    return refuse(err, "rjp_gaincal: h_sol must start at 0, rise in steps of 0 or 1 and end at "
                       "n_sol - 1");
  if (model_maps != 1 && model_maps != n_maps)
    return refuse(err, "rjp_gaincal: model_maps must be 1 or n_maps");
  if (d_w && w_maps != 1 && w_maps != n_maps)
    return refuse(err, "rjp_gaincal: w_maps must be 1 or n_maps");
  if (mode != 0 && mode != 1)
    return refuse(err, "rjp_gaincal: mode must be 0 (amplitude and phase) or 1 (phase only)");
  if (refant < 0 || refant >= n_ant) return refuse(err, "rjp_gaincal: refant outside 0 .. n_ant - 1");
  if (min_bl < 1) return refuse(err, "rjp_gaincal: min_bl < 1");
  if (!(tol > 0.0) || !std::isfinite(tol))
    return refuse(err, "rjp_gaincal: tol must be finite and positive");
  if (n_iter < 1) return refuse(err, "rjp_gaincal: n_iter < 1");
  const int64_t n_bl = (int64_t)n_ant * (n_ant - 1) / 2, n_ms = (int64_t)n_maps * n_sol;
  if ((n_ms * n_bl + 255) / 256 + 2 * n_ms > (int64_t)INT32_MAX)
    return refuse(err, "rjp_gaincal: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_normal_eq takes, in the order it refuses: NULL pointers, counts below 1, n_part, n_sel,
// the derivative stack and selection it needs, n_par, the indices, w_rows, the workgroup count
// (512 samples each).  (`d_w` may be NULL; the workspace is checked where its size lives.)
inline int check_normal_eq(const double* d_data, const double* d_model, const double* d_dmodel,
                           int64_t n_rows, int n_vis, int n_part, int n_par, const int32_t* h_sel,
                           int n_sel, const double* d_w, int64_t w_rows, const double* d_out,
                           const int64_t* d_count, std::string& err) {
  if (!d_data || !d_model || !d_out || !d_count)
    return refuse(err, "rjp_normal_eq: NULL data, model or outputs");
  if (n_rows < 1 || n_vis < 1) return refuse(err, "rjp_normal_eq: n_rows and n_vis must be positive");
  if (n_part != 1 && n_part != 2)
    return refuse(err, "rjp_normal_eq: n_part must be 1 (real) or 2 (complex)");
  if (n_sel < 0 || n_sel > RJP_NORMAL_EQ_MAX_SEL)
    return refuse(err, "rjp_normal_eq: n_sel must lie in 0 .. RJP_NORMAL_EQ_MAX_SEL (" +
                           std::to_string(RJP_NORMAL_EQ_MAX_SEL) + ")");
  if (n_sel > 0 && (!d_dmodel || !h_sel))
    return refuse(err, "rjp_normal_eq: NULL derivatives or selection with n_sel > 0");
  if (n_par < n_sel) return refuse(err, "rjp_normal_eq: n_par < n_sel");
  for (int i = 0; i < n_sel; ++i) {
    if (h_sel[i] < 0 || h_sel[i] >= n_par)
      return refuse(err, "rjp_normal_eq: h_sel outside 0 .. n_par - 1");
    for (int j = 0; j < i; ++j)
      if (h_sel[j] == h_sel[i]) return refuse(err, "rjp_normal_eq: h_sel repeats an index");
  }
  if (d_w && w_rows != 1 && w_rows != n_rows)
    return refuse(err, "rjp_normal_eq: w_rows must be 1 or n_rows");
  if (n_rows > ((int64_t)INT32_MAX * 512) / n_vis)
    return refuse(err, "rjp_normal_eq: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_uv_weights takes, in the order it refuses: NULL pointers, counts below 1, a non-finite
// scale, the mode, the robustness.  (`d_w`, `d_stats` and `d_density` may be NULL; the grids and the
// workspace are checked where the tiling lives.)
inline int check_uv_weights(int n_maps, int n_vis, const double* h_su, const double* h_sv,
                            const double* d_u, const double* d_v, int nx, int nz, int mode,
                            double robust, const double* d_wout, std::string& err) {
  if (!h_su || !h_sv || !d_u || !d_v || !d_wout)
    return refuse(err, "rjp_uv_weights: NULL scales, baselines or output");
  if (n_maps < 1 || n_vis < 1 || nx < 1 || nz < 1)
    return refuse(err, "rjp_uv_weights: n_maps, n_vis, nx and nz must be positive");
  for (int m = 0; m < n_maps; ++m)
    if (!std::isfinite(h_su[m]) || !std::isfinite(h_sv[m]))
      return refuse(err, "rjp_uv_weights: non-finite h_su / h_sv");
  if (mode != 1 && mode != 2)
    return refuse(err, "rjp_uv_weights: mode must be 1 (uniform) or 2 (Briggs)");
  if (mode == 2 && !(robust >= -2.0 && robust <= 2.0))
    return refuse(err, "rjp_uv_weights: robust must be finite and lie in [-2, 2]");
  return RJP_OK;
}

// What rjp_uv_tracks takes, in the order it refuses: NULL pointers, the counts, a non-finite
// position or declination, (sin, cos) off the unit circle, the size of the outputs.  (`d_w` and
// `h_up` may be NULL; a non-finite h_gha[t] is no refusal: it flags integration t.)
inline int check_uv_tracks(const double* h_xyz, int n_ant, const double* h_gha, int n_t,
                           double sin_dec, double cos_dec, const double* d_u, const double* d_v,
                           std::string& err) {
  if (!h_xyz || !h_gha || !d_u || !d_v)
    return refuse(err, "rjp_uv_tracks: NULL positions, hour angles or outputs");
  if (n_ant < 2) return refuse(err, "rjp_uv_tracks: n_ant < 2");
  if (n_t < 1) return refuse(err, "rjp_uv_tracks: n_t < 1");
  for (int64_t i = 0; i < 3 * (int64_t)n_ant; ++i)
    if (!std::isfinite(h_xyz[i])) return refuse(err, "rjp_uv_tracks: non-finite h_xyz");
  if (!std::isfinite(sin_dec) || !std::isfinite(cos_dec))
    return refuse(err, "rjp_uv_tracks: non-finite sin_dec / cos_dec");
  if (!(std::fabs(sin_dec * sin_dec + cos_dec * cos_dec - 1.0) <= 1e-12))
    return refuse(err, "rjp_uv_tracks: sin_dec^2 + cos_dec^2 differs from 1 by more than 1e-12");
  const int64_t n_bl = (int64_t)n_ant * (n_ant - 1) / 2;
  if (n_bl > (int64_t)INT32_MAX / n_t)
    return refuse(err, "rjp_uv_tracks: n_t * n_bl exceeds 2^31 - 1");
  return RJP_OK;
}

// What rjp_vis_noise takes, in the order it refuses: NULL pointers, the counts, the rms values,
// the offsets.  (`d_s` may be NULL.)
inline int check_vis_noise(const double* d_vis, int n_maps, int n_vis, const double* h_sigma,
                           int64_t k0, int32_t m0, const double* d_out, std::string& err) {
  if (!d_vis || !h_sigma || !d_out)
    return refuse(err, "rjp_vis_noise: NULL visibilities, sigmas or output");
  if (n_maps < 1 || n_vis < 1)
    return refuse(err, "rjp_vis_noise: n_maps and n_vis must be positive");
  for (int m = 0; m < n_maps; ++m)
    if (!(h_sigma[m] >= 0.0) || !std::isfinite(h_sigma[m]))
      return refuse(err, "rjp_vis_noise: negative or non-finite h_sigma");
  if (k0 < 0 || k0 > INT64_MAX - (int64_t)n_vis)
    return refuse(err, "rjp_vis_noise: k0 must be >= 0 and k0 + n_vis at most 2^63 - 1");
  if (m0 < 0 || m0 > INT32_MAX - n_maps)
    return refuse(err, "rjp_vis_noise: m0 must be >= 0 and m0 + n_maps at most 2^31 - 1");
  return RJP_OK;
}

// The stack sizes K25's three calls share, in the order they refuse: the counts, the limits of the
// launch grid, the pixel index.
inline int check_region_sizes(const char* who, int n_maps, int nx, int nz, std::string& err) {
  const std::string w = who;
  if (n_maps < 1 || nx < 1 || nz < 1)
    return refuse(err, w + ": n_maps, nx and nz must be positive");
  if (n_maps > RJP_REGIONS_MAX_MAPS)
    return refuse(err, w + ": n_maps exceeds RJP_REGIONS_MAX_MAPS (" +
                           std::to_string(RJP_REGIONS_MAX_MAPS) + ")");
  if (nx > RJP_REGIONS_MAX_NX)
    return refuse(err, w + ": nx exceeds RJP_REGIONS_MAX_NX (" +
                           std::to_string(RJP_REGIONS_MAX_NX) + ")");
  if ((int64_t)nx * nz > (int64_t)INT32_MAX) return refuse(err, w + ": nx * nz exceeds 2^31 - 1");
  return RJP_OK;
}

// What rjp_image_stats takes, in the order it refuses: NULL pointers, the sizes, n_mask with a mask,
// the workgroups.  (`d_mask` may be NULL; `sense` is any integer.)
inline int check_image_stats(const double* d_img, int n_maps, int nx, int nz, const uint8_t* d_mask,
                             int n_mask, const double* d_stats, std::string& err) {
  if (!d_img || !d_stats) return refuse(err, "rjp_image_stats: NULL image or output");
  if (int r = check_region_sizes("rjp_image_stats", n_maps, nx, nz, err)) return r;
  if (d_mask && n_mask != 1 && n_mask != n_maps)
    return refuse(err, "rjp_image_stats: n_mask must be 1 or n_maps");
  if (((int64_t)nx * nz + 2047) / 2048 * n_maps > (int64_t)INT32_MAX)
    return refuse(err, "rjp_image_stats: more than 2^31 - 1 workgroups");
  return RJP_OK;
}

// What rjp_label_regions takes, in the order it refuses: NULL pointers, the sizes, n_mask, the
// connectivity.  (`d_area` may be NULL.)
inline int check_label_regions(const uint8_t* d_mask_in, int n_mask, int n_maps, int nx, int nz,
                               int connectivity, const int32_t* d_label, const int32_t* d_nreg,
                               std::string& err) {
  if (!d_mask_in || !d_label || !d_nreg) return refuse(err, "rjp_label_regions: NULL mask or outputs");
  if (int r = check_region_sizes("rjp_label_regions", n_maps, nx, nz, err)) return r;
  if (n_mask != 1 && n_mask != n_maps)
    return refuse(err, "rjp_label_regions: n_mask must be 1 or n_maps");
  if (connectivity != 1 && connectivity != 2)
    return refuse(err, "rjp_label_regions: connectivity must be 1 (four neighbours) or 2 (eight)");
  return RJP_OK;
}

// What rjp_mask_grow takes, in the order it refuses: NULL pointers, the sizes, n_mask, the
// connectivity.  (`n_iter` is any integer: 0 nothing, > 0 that many steps, < 0 until stable.)
inline int check_mask_grow(const uint8_t* d_seed, const uint8_t* d_con, int n_mask, int n_maps,
                           int nx, int nz, int connectivity, std::string& err) {
  if (!d_seed || !d_con) return refuse(err, "rjp_mask_grow: NULL seed or constraint");
  if (int r = check_region_sizes("rjp_mask_grow", n_maps, nx, nz, err)) return r;
  if (n_mask != 1 && n_mask != n_maps)
    return refuse(err, "rjp_mask_grow: n_mask must be 1 or n_maps");
  if (connectivity != 1 && connectivity != 2)
    return refuse(err, "rjp_mask_grow: connectivity must be 1 (four neighbours) or 2 (eight)");
  return RJP_OK;
}

}  // namespace rjp_args
