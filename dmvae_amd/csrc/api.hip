// C-ABI plumbing: thread-local error string + version.
#include "common.h"
#include "dmvae_hip.h"
#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512] = "";

void dmvae_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int dmvae_lds_optin(dmvae_lds_seen* seen, const void* kernel, int bytes, const char* file, int line) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev < 63 ? dev : 63);
  if (e == hipSuccess && dev < 63 && (__atomic_load_n(&seen->devs, __ATOMIC_RELAXED) & bit)) return 0;
  if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // reported here: the next entry point's DMVAE_CHECK_LAUNCH must not find it
    dmvae_set_error("%s:%d: %d bytes of dynamic LDS refused on device %d: %s", file, line, bytes, dev, hipGetErrorString(e));
    return -5;
  }
  __atomic_fetch_or(&seen->devs, bit, __ATOMIC_RELAXED);
  return 0;
}

extern "C" const char* dmvae_last_error(void) { return g_err; }
extern "C" int dmvae_abi_version(void) { return 9; }   // 9: the retired split-K pair and NULL-statistics aliases removed; 8: dmvae_reparam_kl_* (the reparameterise hook + posterior-form KL); 7: the XCD-placed grouped weight-gradient launch (dmvae_linear_wgrad_grouped_plan / _xcd); 6: the whole-stack DiT backward + batched per-sample Linears + batched weight transposes; 5: the shortcut-in-GroupNorm entry points (dmvae_groupnorm_*_short); 2: dmvae_conv_desc gained w_layout; 3: dmvae_pack_entry + the batched pack / Linear GEMM entry points; 4: the decoder-tail entry points (dmvae_norm_conv_out_*)
