// dmx_internal.h -- shared declarations of libdemux_hip.so (not part of the public ABI).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "demux_hip.h"
#include "demux_hip_debug.h"

namespace dmx {

constexpr int COVERAGE_STAGES = 6;     // stages dmx_coverage_count (4) and dmx_coverage_candidates (2) time (coverage.hip; dmx_get_coverage_timings)
constexpr int COUNT_READS_STAGES = 7;  // stages dmx_count_reads times (count_reads.hip; dmx_get_count_reads_timings fills that many)

// records a message for dmx_last_error() and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace dmx
