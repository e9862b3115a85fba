// segment_checks.h -- the rules of a segment's offsets and firsts as the host forms of the segment calls check them before anything is
// copied (segment_lists.hip.h has the device form's): 64-bit offsets from 0, never backwards, no item of 4 GiB; 32-bit firsts from 0 to
// their total, never backwards.  Plain host C++, nothing of HIP: tests/native compiles it into stand-alone programs.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"

namespace phant {
namespace seg {

// Host form: "<call>: <array> ..." in err; the offsets end where their last entry says (`item`: what one of them holds)
inline int32_t check_offsets_host(const char* call, const char* array, const char* item, const uint64_t* off, uint32_t n, std::string& err) {
    if (off[0] != 0u) return err = std::string(call) + ": " + array + " does not run from 0", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1u] < off[i]) return err = std::string(call) + ": " + array + " goes backwards", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1u] - off[i] > 0xffffffffull) return err = std::string(call) + ": a " + item + " of 4 GiB or more", PHANT_E_UNSUPPORTED;
    return PHANT_OK;
}
inline int32_t check_firsts_host(const char* call, const char* array, const char* to, const uint32_t* first, uint32_t n, uint32_t total, std::string& err) {
    if (first[0] != 0u || first[n] != total) return err = std::string(call) + ": " + array + " does not run from 0 to " + to, PHANT_E_INVALID_ARG;
    for (uint32_t b = 0; b < n; ++b)
        if (first[b + 1u] < first[b]) return err = std::string(call) + ": " + array + " goes backwards", PHANT_E_INVALID_ARG;
    return PHANT_OK;
}

}  // namespace seg
}  // namespace phant
