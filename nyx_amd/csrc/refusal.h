// refusal.h - a refusal as data (host only, no HIP): what the pure check functions of series_host.h, chain_args.h, lambert_args.h,
// target_args.h, run_host.h and stats_host.h return, and abi.cpp hands to nyx_set_error.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/nyx_hip.h"

// The return code and the message.  rc == NYX_HIP_RC_OK: accepted.
struct Refusal {
    int rc = NYX_HIP_RC_OK;
    char msg[256] = "";
    explicit operator bool() const { return rc != NYX_HIP_RC_OK; }
};
__attribute__((format(printf, 1, 2))) inline Refusal bad_arg(const char *fmt, ...) {
    Refusal r;
    r.rc = NYX_HIP_RC_BAD_ARG;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof r.msg, fmt, ap);
    va_end(ap);
    return r;
}
