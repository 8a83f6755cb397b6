// tool_base.hpp -- what every part of mdbg_tool leans on: how it dies, its library contexts, the phase trace.
#pragma once
#include <sys/time.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mdbg_hip.h"

// _exit, not exit: with --gpus G a failing rank thread ends the process while its peers may sit inside an RCCL collective
// waiting for it; exit() would run the static destructors of HIP / RCCL under them and can hang, and the parent
// (Utils::executeCommand, Commons.hpp:2855) only needs the non-zero status.  Output files are flushed as they are written.
[[noreturn]] inline void die(const std::string &msg) {
    fprintf(stderr, "mdbg_tool: %s\n", msg.c_str());
    fflush(nullptr);
    _exit(1);
}

inline mdbg_ctx *g_ctx = nullptr;
inline std::vector<mdbg_ctx *> g_more_ctx;      // the other consumers' contexts (readSelection)

// phase timings on stderr when MDBG_TRACE is set
struct Trace {
    double t0;
    static double now() { struct timeval tv; gettimeofday(&tv, nullptr); return tv.tv_sec + 1e-6 * tv.tv_usec; }
    Trace() : t0(now()) {}
    void mark(const char *what) { if (getenv("MDBG_TRACE")) fprintf(stderr, "[mdbg_tool] %8.3f s  %s\n", now() - t0, what); }
    void mark(const std::string &what) { mark(what.c_str()); }
};
inline Trace g_trace;

inline void check(int rc, const char *what) {
    if (rc != MDBG_OK) die(std::string(what) + ": " + mdbg_last_error(g_ctx));
}
inline void check_on(mdbg_ctx *ctx, int rc, const char *what) {
    if (rc) die(std::string(what) + ": " + mdbg_last_error(ctx));
}
