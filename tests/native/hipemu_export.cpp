// Part of libphant_emu.so only (tests/emu.py): lets a test read the emulator's counters.
#include <hip/hip_runtime.h>

extern "C" __attribute__((visibility("default"))) unsigned long long hipemu_graph_launches(void) {
    return hipemu::M.graph_launches;
}

extern "C" __attribute__((visibility("default"))) void hipemu_counters(unsigned long long out[3]) {
    out[0] = hipemu::M.launches;
    out[1] = hipemu::M.wave_ops;       // cross-lane operations resolved
    out[2] = hipemu::M.divergent_ops;  // ... of which with an active mask smaller than the wave's live lanes
}

// hipMemcpyAsync calls host to device, device to host and device to device, hipMemsetAsync calls, hipStreamSynchronize calls
extern "C" __attribute__((visibility("default"))) void hipemu_bus_counters(unsigned long long out[5]) {
    out[0] = hipemu::M.h2d;
    out[1] = hipemu::M.d2h;
    out[2] = hipemu::M.d2d;
    out[3] = hipemu::M.memsets;
    out[4] = hipemu::M.stream_syncs;
}

// radix_sort.hip's prefix sum over caller-supplied counters (test hook: the product's C-ABI reaches it only inside its callers -- headers,
// receipts, transactions, access lists, the post-state and, three times, the state root; phant_diag_scan_u32 is the same offer
// through the C-ABI, with guards behind the buffers).
#include "../../phant_amd/csrc/launch.h"
extern "C" __attribute__((visibility("default"))) int hipemu_test_exclusive_scan(unsigned* counters, unsigned n) {
    unsigned *d = nullptr, *scratch = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), 4ull * n + 64) != hipSuccess) return -1;
    if (hipMalloc(reinterpret_cast<void**>(&scratch), 4 * phant::scan_scratch_entries(n) + 64) != hipSuccess) return -1;
    int rc = 0;
    if (hipMemcpy(d, counters, 4ull * n, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    if (!rc && phant::launch_exclusive_scan_u32(d, n, scratch, nullptr) != hipSuccess) rc = -3;
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = -4;
    if (!rc && hipMemcpy(counters, d, 4ull * n, hipMemcpyDeviceToHost) != hipSuccess) rc = -5;
    (void)hipFree(d);
    (void)hipFree(scratch);
    return rc;
}
