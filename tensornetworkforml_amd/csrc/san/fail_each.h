// Shared by the sanitizer mains: every allocation of a call fails in turn (san_stub_fail_alloc of hip_stub.cpp).
#pragma once
#include <cstdio>
#include <cstdlib>
#include "../../../include/tnml.h"

extern "C" long san_stub_alloc_calls(void);
extern "C" void san_stub_fail_alloc(long nth);
extern "C" int san_stub_fail_pending(void);

// call() -> a tnml status.  For k = 1, 2, ... the k-th allocation call inside it fails: it must report TNML_ERR_HIP, and the context
// must take the same call again.  The first run the failure does not fire in (the call made fewer than k allocations) is that call
// repeated without a failure: it must succeed.  -> the number of allocations that failed in turn
template <class F> static int fail_each_alloc(const char *what, F call) {
  for (int k = 1;; ++k) {
    san_stub_fail_alloc(k);
    const int rc = call();
    if (san_stub_fail_pending()) {
      san_stub_fail_alloc(0);
      if (rc != TNML_OK) { fprintf(stderr, "%s: repeated without a failure -> %d: %s\n", what, rc, tnml_last_error()); exit(1); }
      printf("failed allocations, %-44s %2d failed in turn, each TNML_ERR_HIP; then ok\n", what, k - 1);
      fflush(stdout);
      return k - 1;
    }
    if (rc != TNML_ERR_HIP) { fprintf(stderr, "%s: allocation %d failed, the call returned %d (%s)\n", what, k, rc, rc ? tnml_last_error() : "ok"); exit(1); }
  }
}
