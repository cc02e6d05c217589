// The library's switches: environment variables named HRY_*, every one listed in INTEGRATION.md.  One parse rule for all:
// a flag is on when it is set to anything but "" or "0"; a number is a decimal, and dflt when the variable is unset or "".
// Each call reads the environment afresh; a site that reads a switch once per process keeps the value in a static of its own.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace hry {

inline bool env_on(const char *name)
{
	const char *e = getenv(name);
	return e && *e && !(e[0] == '0' && e[1] == 0);
}

constexpr uint64_t kEnvUnset = ~0ull;   // a default for env_uint where "unset" means something of its own

inline uint64_t env_uint(const char *name, uint64_t dflt)
{
	const char *e = getenv(name);
	return e && *e ? (uint64_t)strtoull(e, nullptr, 10) : dflt;
}

// HRY_TRACE: wall-clock marks of the encode and the decode on stderr (development aid), read once
inline bool trace_on()
{
	static const bool on = env_on("HRY_TRACE");
	return on;
}

}   // namespace hry
