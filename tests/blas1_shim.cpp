// Test shim: reaches the vector-kernel and Lanczos-fold launchers of csrc/kernels_blas1.hip from ctypes.  The launchers are ordinary C++
// functions of libspindyn.so (declared in csrc/sd_internal.hpp, default visibility, not in include/spindyn.h); this unit
// forward-declares the ones it needs -- prototypes copied from sd_internal.hpp -- and wraps each in an extern "C" function that
// takes the context as void *.  It includes no HIP header.  The mangled names carry the parameter types, so a prototype that
// drifts from the library fails to link (-Wl,--no-undefined): the link step is the signature check.
#include <cstdint>

struct sd_ctx;

int sd_k_gs_blocks(int64_t N);
int sd_k_lanczos_fold_blocks(int64_t N);
int sd_k_gs_chain(sd_ctx *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, const double *y, double *scratch,
                  double *alpha_part, double *chk_dev);
int sd_k_gs_update(sd_ctx *ctx, double *w, const double *vj, const double *vjm1, int64_t N, const double *alpha_part,
                   const double *n2_prev, double *store_alpha, double *store_beta, double *n2_out, double *upd_scratch);
int sd_k_gs_scale(sd_ctx *ctx, double *vnext, const double *w, int64_t N, const double *n2_part, double *store_beta);
int sd_k_mgs_chain(sd_ctx *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, int slot);
int sd_k_bgs_chain(sd_ctx *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, int slot);
int sd_read_scalars(sd_ctx *ctx, int slot, int count, double *out);
int sd_k_mdot(sd_ctx *ctx, const double *V, int64_t ld, int ncols, const double *y, int64_t N, double *out_host);
int sd_k_gemv_cols(sd_ctx *ctx, double *y, const double *V, int64_t N, int ncols, const double *coef_host);
int sd_k_ccombine(sd_ctx *ctx, double *y, const double *const *cols, int64_t N, int ncols, const double *cr, const double *ci);
int sd_k_cheb_init(sd_ctx *ctx, double *y, const double *x0, const double *x1, int64_t N, double c0r, double c0i, double c1r,
                   double c1i, int have1);
int sd_k_promote(sd_ctx *ctx, double *yc, const double *x, int nc_in, int64_t N);
int sd_k_sub2(sd_ctx *ctx, double *w, const double *v, const double *u, int64_t n, double a, double b);
int sd_k_scale_div(sd_ctx *ctx, double *y, const double *x, int64_t n, double d);
int sd_k_dotu(sd_ctx *ctx, const double *x, const double *y, int64_t N, int slot);
int sd_k_imag_count(sd_ctx *ctx, const double *xc, int64_t N, int slot);
int sd_k_dot_to(sd_ctx *ctx, int nc, const double *x, const double *y, int64_t N, double *dst_dev);
int sd_k_nrm2sq_to(sd_ctx *ctx, const double *x, int64_t n, double *dst_dev);
int sd_k_lanczos_fold(sd_ctx *ctx, double *t, const double *uc, const double *up, int64_t N, int form, const double *dot_dev,
                      const double *n2c_dev, const double *n2p_dev, double *store_alpha, double *store_bc, double *n2_out);
int sd_k_lanczos_fold_p(sd_ctx *ctx, double *t, const double *uc, const double *up, int64_t N, int batch, int64_t bstride, int form,
                        const double *dotp, int ndot, const double *n2cp, const double *n2pp, int nn2, double *store_alpha,
                        double *store_bc, int64_t store_stride, double *n2out, int nb);
int sd_k_lanczos_fold_scalars_p(sd_ctx *ctx, int batch, int form, const double *dotp, int ndot, const double *n2cp, int nn2,
                                double *store_alpha, double *store_bc, int64_t store_stride);
int sd_k_lanczos_fold_scalars(sd_ctx *ctx, int form, const double *dot_dev, const double *n2c_dev, double *store_alpha,
                              double *store_bc);

extern "C" {

int sd_device_count(void);   // include/spindyn.h: the address both sides must agree on (one loaded instance of the library)
void *b1_addr_of_sd_device_count(void) { return reinterpret_cast<void *>(&sd_device_count); }

int b1_gs_blocks(int64_t N) { return sd_k_gs_blocks(N); }
int b1_lanczos_fold_blocks(int64_t N) { return sd_k_lanczos_fold_blocks(N); }
int b1_gs_chain(void *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, const double *y, double *scratch,
                double *alpha_part, double *chk_dev) {
  return sd_k_gs_chain(static_cast<sd_ctx *>(ctx), w, V, ld, ncols, N, y, scratch, alpha_part, chk_dev);
}
int b1_gs_update(void *ctx, double *w, const double *vj, const double *vjm1, int64_t N, const double *alpha_part,
                 const double *n2_prev, double *store_alpha, double *store_beta, double *n2_out, double *upd_scratch) {
  return sd_k_gs_update(static_cast<sd_ctx *>(ctx), w, vj, vjm1, N, alpha_part, n2_prev, store_alpha, store_beta, n2_out, upd_scratch);
}
int b1_gs_scale(void *ctx, double *vnext, const double *w, int64_t N, const double *n2_part, double *store_beta) {
  return sd_k_gs_scale(static_cast<sd_ctx *>(ctx), vnext, w, N, n2_part, store_beta);
}
int b1_mgs_chain(void *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, int slot) {
  return sd_k_mgs_chain(static_cast<sd_ctx *>(ctx), w, V, ld, ncols, N, slot);
}
int b1_bgs_chain(void *ctx, double *w, const double *V, int64_t ld, int ncols, int64_t N, int slot) {
  return sd_k_bgs_chain(static_cast<sd_ctx *>(ctx), w, V, ld, ncols, N, slot);
}
int b1_read_scalars(void *ctx, int slot, int count, double *out) {
  return sd_read_scalars(static_cast<sd_ctx *>(ctx), slot, count, out);
}
int b1_mdot(void *ctx, const double *V, int64_t ld, int ncols, const double *y, int64_t N, double *out_host) {
  return sd_k_mdot(static_cast<sd_ctx *>(ctx), V, ld, ncols, y, N, out_host);
}
int b1_gemv_cols(void *ctx, double *y, const double *V, int64_t N, int ncols, const double *coef_host) {
  return sd_k_gemv_cols(static_cast<sd_ctx *>(ctx), y, V, N, ncols, coef_host);
}
int b1_ccombine(void *ctx, double *y, const double *const *cols, int64_t N, int ncols, const double *cr, const double *ci) {
  return sd_k_ccombine(static_cast<sd_ctx *>(ctx), y, cols, N, ncols, cr, ci);
}
int b1_cheb_init(void *ctx, double *y, const double *x0, const double *x1, int64_t N, double c0r, double c0i, double c1r,
                 double c1i, int have1) {
  return sd_k_cheb_init(static_cast<sd_ctx *>(ctx), y, x0, x1, N, c0r, c0i, c1r, c1i, have1);
}
int b1_promote(void *ctx, double *yc, const double *x, int nc_in, int64_t N) {
  return sd_k_promote(static_cast<sd_ctx *>(ctx), yc, x, nc_in, N);
}
int b1_sub2(void *ctx, double *w, const double *v, const double *u, int64_t n, double a, double b) {
  return sd_k_sub2(static_cast<sd_ctx *>(ctx), w, v, u, n, a, b);
}
int b1_scale_div(void *ctx, double *y, const double *x, int64_t n, double d) {
  return sd_k_scale_div(static_cast<sd_ctx *>(ctx), y, x, n, d);
}
int b1_dotu(void *ctx, const double *x, const double *y, int64_t N, int slot) {
  return sd_k_dotu(static_cast<sd_ctx *>(ctx), x, y, N, slot);
}
int b1_imag_count(void *ctx, const double *xc, int64_t N, int slot) {
  return sd_k_imag_count(static_cast<sd_ctx *>(ctx), xc, N, slot);
}
int b1_dot_to(void *ctx, int nc, const double *x, const double *y, int64_t N, double *dst_dev) {
  return sd_k_dot_to(static_cast<sd_ctx *>(ctx), nc, x, y, N, dst_dev);
}
int b1_nrm2sq_to(void *ctx, const double *x, int64_t n, double *dst_dev) {
  return sd_k_nrm2sq_to(static_cast<sd_ctx *>(ctx), x, n, dst_dev);
}
int b1_lanczos_fold(void *ctx, double *t, const double *uc, const double *up, int64_t N, int form, const double *dot_dev,
                    const double *n2c_dev, const double *n2p_dev, double *store_alpha, double *store_bc, double *n2_out) {
  return sd_k_lanczos_fold(static_cast<sd_ctx *>(ctx), t, uc, up, N, form, dot_dev, n2c_dev, n2p_dev, store_alpha, store_bc, n2_out);
}
int b1_lanczos_fold_p(void *ctx, double *t, const double *uc, const double *up, int64_t N, int batch, int64_t bstride, int form,
                      const double *dotp, int ndot, const double *n2cp, const double *n2pp, int nn2, double *store_alpha,
                      double *store_bc, int64_t store_stride, double *n2out, int nb) {
  return sd_k_lanczos_fold_p(static_cast<sd_ctx *>(ctx), t, uc, up, N, batch, bstride, form, dotp, ndot, n2cp, n2pp, nn2, store_alpha,
                             store_bc, store_stride, n2out, nb);
}
int b1_lanczos_fold_scalars_p(void *ctx, int batch, int form, const double *dotp, int ndot, const double *n2cp, int nn2,
                              double *store_alpha, double *store_bc, int64_t store_stride) {
  return sd_k_lanczos_fold_scalars_p(static_cast<sd_ctx *>(ctx), batch, form, dotp, ndot, n2cp, nn2, store_alpha, store_bc,
                                     store_stride);
}
int b1_lanczos_fold_scalars(void *ctx, int form, const double *dot_dev, const double *n2c_dev, double *store_alpha, double *store_bc) {
  return sd_k_lanczos_fold_scalars(static_cast<sd_ctx *>(ctx), form, dot_dev, n2c_dev, store_alpha, store_bc);
}

}  // extern "C"
