// What the host code asks of the CURRENT device, answered in one place ("Caches: by tensor object, by memory stamp,
// by device").  Host only.  Everything here is kept PER DEVICE: a process may drive several devices, or partitions with
// different compute-unit counts, and a function's attributes belong to the function on one device.  The functions are inline
// with function-local statics, so the library has one table, not one per translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>

#include "geom_hip.h"

namespace geom {

constexpr int MAX_DEVICES = 64;

struct DeviceFacts {
    int device;                 // its index: what a caller keys a per-device number of its own on
    int compute_units;          // > 0
    size_t lds_per_block_optin; // the most LDS one workgroup can be granted (the largest of the three fields the runtime reports)
};

// The facts of the current device: filled once per device per process, from one property query; every later call costs one
// hipGetDevice.  nullptr when the device is unknown (no device, an index beyond the table, a failed query) -- a failure is
// not remembered, and every caller has its own answer for it.
inline const DeviceFacts *device_facts()
{
    static DeviceFacts facts[MAX_DEVICES]; // compute_units == 0: not filled yet
    static std::mutex filling;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(filling);
    if (!facts[dev].compute_units) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return nullptr;
        size_t lds = prop.sharedMemPerBlock;
        if (prop.sharedMemPerBlockOptin > lds) lds = prop.sharedMemPerBlockOptin;
        if (prop.maxSharedMemoryPerMultiProcessor > lds) lds = prop.maxSharedMemoryPerMultiProcessor;
        facts[dev] = DeviceFacts{dev, prop.multiProcessorCount, lds};
    }
    return &facts[dev];
}

// Let `kernel` take up to `bytes` of dynamic LDS on device `on` (default: the current one); done once per (kernel, device) and
// again only for a larger request.  0, or GEOM_EINVAL when the runtime refuses.  An unknown device is left alone: the launch
// reports what is wrong with it.
inline int allow_dynamic_lds_of(const void *kernel, int bytes, const DeviceFacts *on)
{
    struct Granted {
        const void *kernel;
        int bytes[MAX_DEVICES];
    };
    static Granted granted[16]; // (the library has four such kernels; a seventeenth would ask the runtime at every call)
    static std::mutex granting;
    if (!on) return 0;
    std::lock_guard<std::mutex> lock(granting);
    Granted *g = granted;
    while (g != granted + 16 && g->kernel && g->kernel != kernel) ++g;
    if (g != granted + 16 && g->kernel && g->bytes[on->device] >= bytes) return 0;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return GEOM_EINVAL;
    if (g != granted + 16) g->kernel = kernel, g->bytes[on->device] = bytes;
    return 0;
}
template <class Kernel>
int allow_dynamic_lds(Kernel kernel, int bytes, const DeviceFacts *on = device_facts())
{
    return allow_dynamic_lds_of(reinterpret_cast<const void *>(kernel), bytes, on);
}

} // namespace geom
