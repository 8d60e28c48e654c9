// gcm_kernels13.hip — the T-table and split batch kernels for TLS 1.3 session
// tables: gcm_kernels.hip compiled for the RFC 8446 record layout (TG_TLS13,
// gcm_device.h).  Launchers: launch_gcm13, launch_gcm_split13.
#define TG_TLS13 1
#include "gcm_kernels.hip"
