// Makes a device current for a scope and puts the caller's back on the way out, so an entry
// point returns from anywhere with a plain `return`.  A caller already on that device pays one
// hipGetDevice and nothing else.  Shared by the WebSocket engine (ws_gpu.hip) and the TLS
// engine (tls_gpu.hip).
#ifndef UVHTTP_DEVICE_GUARD_H
#define UVHTTP_DEVICE_GUARD_H

#include <hip/hip_runtime.h>

struct DeviceGuard {
    int device, prev;
    explicit DeviceGuard(int dev) : device(dev), prev(0) {
        (void)hipGetDevice(&prev);
        if (prev != device) (void)hipSetDevice(device);
    }
    // the second half of a switch made by an earlier guard that was kept (keep): only restores
    DeviceGuard(int dev, int kept_prev) : device(dev), prev(kept_prev) {}
    ~DeviceGuard() {
        if (prev != device) (void)hipSetDevice(prev);
    }
    // leaves `device` current past the scope; returns the device to restore later
    int keep() {
        const int p = prev;
        prev = device;
        return p;
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#endif
