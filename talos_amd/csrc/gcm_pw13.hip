// gcm_pw13.hip — the per-wave-session kernel for TLS 1.3 session tables:
// gcm_pw.hip compiled for the RFC 8446 record layout (TG_TLS13, gcm_device.h;
// DESIGN.md §4.14).  Launcher: launch_gcm_pw13.
#define TG_TLS13 1
#include "gcm_pw.hip"
