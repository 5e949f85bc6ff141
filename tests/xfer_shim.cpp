// Test shim: reaches the host <-> device transfer functions of csrc/xfer.cpp from ctypes, at any byte count and any address.  They
// are ordinary C++ functions of libspindyn.so (declared in csrc/sd_internal.hpp, default visibility, not in include/spindyn.h); this
// unit forward-declares them -- prototypes copied from sd_internal.hpp -- and wraps each in an extern "C" function that takes the
// context as void *.  It includes no HIP header.  The mangled names carry the parameter types, so a prototype that drifts from the
// library fails to link (-Wl,--no-undefined): the link step is the signature check.
#include <cstddef>

struct sd_ctx;

int sd_xfer_h2d(sd_ctx *ctx, void *dev, const void *host, size_t bytes);
int sd_xfer_d2h(sd_ctx *ctx, void *host, const void *dev, size_t bytes);
void sd_xfer_release(sd_ctx *ctx);

extern "C" {

int sd_device_count(void);   // include/spindyn.h: the address both sides must agree on (one loaded instance of the library)
void *xf_addr_of_sd_device_count(void) { return reinterpret_cast<void *>(&sd_device_count); }

int xf_h2d(void *ctx, void *dev, const void *host, size_t bytes) { return sd_xfer_h2d(static_cast<sd_ctx *>(ctx), dev, host, bytes); }
int xf_d2h(void *ctx, void *host, const void *dev, size_t bytes) { return sd_xfer_d2h(static_cast<sd_ctx *>(ctx), host, dev, bytes); }
// frees the pinned ring, its events and the team; the caller has no transfer in flight (both functions above complete on return)
void xf_release(void *ctx) { sd_xfer_release(static_cast<sd_ctx *>(ctx)); }

}  // extern "C"
