// sim_common.h -- what the CPU logic checkers of the banded kernels share (TEST INFRASTRUCTURE): reading the case file, walking
// the waves of a launch that the kernel's plan describes, writing the canvas.
#pragma once

#include <stdio.h>
#include <string.h>

#include <vector>

#include "../h263-rs_amd/csrc/band_launch.h"

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

// the canvas after the launch -> `path`; the main's exit status
static int write_canvas(const char *path, const std::vector<uint8_t> &canvas, const void *more = nullptr, size_t more_bytes = 0)
{
    FILE *out = fopen(path, "wb");
    if (!out || fwrite(canvas.data(), 1, canvas.size(), out) != canvas.size()) return 2;
    if (more_bytes && fwrite(more, 1, more_bytes, out) != more_bytes) return 2;
    fclose(out);
    return 0;
}

// The waves of the launch `d` in grid order (y = picture or region, z = column segment, x = XCD-ordered band): a band beyond the
// last one leaves as the kernel's wrapper does; the LDS and the 64 lanes are poisoned in front of every wave, and item(lds, band,
// z, y, each) runs it with each(f) = f(lane, lane_state) over the 64 lanes in turn.
template <class Lds, class Lane, class Item>
static void run_banded(const h263mi::LaunchDims &d, uint32_t bands, uint32_t chunk, Item item)
{
    static Lds lds;
    static Lane lanes[64];
    auto each = [&](auto f) {
        for (int l = 0; l < 64; l++) f(l, lanes[l]);
    };
    for (uint32_t y = 0; y < d.y; y++)
        for (uint32_t z = 0; z < d.z; z++)
            for (uint32_t x = 0; x < d.x; x++) {
                const uint32_t band = h263mi::xcd_band(x, chunk);
                if (band >= bands) continue;
                memset(&lds, 0xA5, sizeof lds);
                memset(lanes, 0x5A, sizeof lanes);
                item(lds, band, z, y, each);
            }
}
