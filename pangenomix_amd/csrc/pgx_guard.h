// The exception guard of the C ABI (pgx.h: "no exception crosses the ABI"), for every translation unit of libpgx,
// the ones compiled without HIP included: it needs pgx.h and pgx_set_error only.
#pragma once
#include <exception>
#include <new>

#include "../../include/pgx.h"

void pgx_set_error(const char *fmt, ...);

// Every entry point of the C ABI that can throw (host allocations, threads) runs its body inside this guard.
template <typename F>
int guarded(const char *fn, F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        pgx_set_error("%s: out of host memory", fn);
        return PGX_ERR_NOMEM;
    } catch (const std::exception &e) {
        pgx_set_error("%s: %s", fn, e.what());
        return PGX_ERR_INTERNAL;
    } catch (...) {
        pgx_set_error("%s: unexpected exception", fn);
        return PGX_ERR_INTERNAL;
    }
}

// The same for an entry point written as a function-try-block: `} catch (...) { return guarded_catch(__func__); }`
// (the exception being handled is thrown again inside the guard).
inline int guarded_catch(const char *fn) {
    return guarded(fn, []() -> int { throw; });
}
