// gcm_queue13.hip — the prep pass and the queue kernel for TLS 1.3 session
// tables: gcm_queue.hip compiled for the RFC 8446 record layout (TG_TLS13,
// gcm_device.h).  Launchers: launch_gcm_prep13, launch_gcm_queue13.
#define TG_TLS13 1
#include "gcm_queue.hip"
