// What the two host programs of the device FFV1 decoder's core share (ffv1_decode_host.cpp, ffv1_stream_decode_host.cpp): the
// asserting byte accessors, the tables the kernels keep in LDS, the CRC of a slice, the store of a decoded row and the job reader.
#pragma once

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mdvt_ffv1_core.h"

using namespace mdvt_ffv1;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "bound violated: %s (line %d)\n", #c, __LINE__); abort(); } } while (0)

struct CheckedSrc {
    const uint8_t* p; uint32_t avail;
    uint8_t byte(uint32_t k) const { CHECK(k < avail); return p[k]; }
};

struct CheckedPacket {
    const uint8_t* p; uint32_t size;
    uint8_t operator()(uint32_t k) const { CHECK(k < size); return p[k]; }
};

struct Tables {
    int8_t q11[256];
    uint16_t next[256];
    Tables()
    {
        uint8_t zero[256], one[256];
        default_states(zero, one);
        for (int k = 0; k < 256; ++k) { q11[k] = (int8_t)quant11(k); next[k] = (uint16_t)(zero[k] | (one[k] << 8)); }
    }
};

// the CRC-32 of packet bytes [off, off + n): zero for an intact slice with its trailer
static inline uint32_t slice_crc(CheckedPacket pkt, uint32_t off, uint32_t n)
{
    uint32_t crc = 0;
    for (uint32_t k = 0; k < n; ++k) crc = (crc << 8) ^ crc_table_entry((crc >> 24) ^ pkt(off + k));
    return crc;
}

// row y of the slice d has just decoded -> its pixels of the W-wide frame at dst
template <class Dec>
static inline void store_row(const Dec& d, int y, uint8_t* dst, int W, int ri, int bi)
{
    const int16_t* l = d.lines + (size_t)(y % 3) * d.stride + 1;
    uint8_t* o = dst + ((size_t)(d.y0 + y) * W + d.x0) * 3;
    for (int x = 0; x < d.sw; ++x) store_rct_pixel(l[x], l[(size_t)3 * d.stride + x], l[(size_t)6 * d.stride + x], o, 3 * x + ri, 3 * x + 1, 3 * x + bi);
}

static inline bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
