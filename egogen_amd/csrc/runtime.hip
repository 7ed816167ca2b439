// What the whole library shares behind the C ABI of include/egogen_hip.h: the thread's last error message, the ABI version and the
// event helpers of the timing calls.
#include "egx_common.h"

static thread_local std::string g_last_error;
void egx_set_error(const std::string& msg) { g_last_error = msg; }
extern "C" const char* egx_last_error(void) { return g_last_error.c_str(); }
extern "C" int egx_version(void) { return 1; }

extern "C" int egx_event_create(void** out_event) {
  EGX_REQUIRE(out_event, "null argument");
  hipEvent_t e;
  EGX_HIP_CHECK(hipEventCreate(&e));
  *out_event = e;
  return EGX_OK;
}
extern "C" int egx_event_destroy(void* event) {
  if (event) EGX_HIP_CHECK(hipEventDestroy(static_cast<hipEvent_t>(event)));
  return EGX_OK;
}
extern "C" int egx_event_elapsed_ms(void* start_event, void* stop_event, float* out_ms) {
  EGX_REQUIRE(start_event && stop_event && out_ms, "null argument");
  EGX_HIP_CHECK(hipEventSynchronize(static_cast<hipEvent_t>(stop_event)));
  EGX_HIP_CHECK(hipEventElapsedTime(out_ms, static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event)));
  return EGX_OK;
}
