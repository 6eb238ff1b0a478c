// fd_jpeg_host.h — the serial half of the baseline JPEG decoder: marker parsing and Huffman decoding on the
// host.  Header-only C++, no HIP, no global state, nothing written but the caller's buffers: fd_jpeg.hip compiles the two
// functions into the library (FD_JPEG_API defined there), tests/abi/jpeg_host_check.cpp includes this file alone and runs them
// under the host sanitizers.  Every read is bounded by `n`, every write by `coef_bytes`; a failure is a return code
// (FD_JPEG_E_* of fcosdet.h), never a message in shared storage, so both functions may run on any number of threads at once.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/fcosdet.h"

#ifndef FD_JPEG_API
#define FD_JPEG_API inline
#endif

// natural (row-major) index of the k-th coefficient in zigzag order
static const uint8_t fd_jpeg_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static inline int32_t fd_jpeg_unsupported(fd_jpeg_info* info, int32_t reason) {
    info->supported = 0;
    info->reason = reason;
    return FD_OK;
}

extern "C" FD_JPEG_API int32_t fd_jpeg_parse(const uint8_t* data, int64_t n, fd_jpeg_info* info) {
    if (!data || !info || n < 0) return FD_JPEG_E_BUFFER;
    memset(info, 0, sizeof(*info));
    if (n < 2) return FD_JPEG_E_TRUNCATED;
    if (data[0] != 0xFF || data[1] != 0xD8) return FD_JPEG_E_MARKER;
    uint16_t qtabs[4][64];
    uint8_t q_defined[4] = {0, 0, 0, 0}, q_wide[4] = {0, 0, 0, 0};
    int32_t comp_id[FD_JPEG_MAX_COMP] = {0, 0, 0}, comp_tq[FD_JPEG_MAX_COMP] = {0, 0, 0};
    int have_sof = 0, have_jfif = 0, adobe_transform = -1;
    int64_t pos = 2;
    for (;;) {
        if (pos >= n) return FD_JPEG_E_TRUNCATED;
        if (data[pos] != 0xFF) return FD_JPEG_E_MARKER;
        while (pos < n && data[pos] == 0xFF) ++pos;          // fill bytes in front of a marker
        if (pos >= n) return FD_JPEG_E_TRUNCATED;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue; // TEM, stray RSTn: no segment
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return FD_JPEG_E_MARKER;
        if (pos + 2 > n) return FD_JPEG_E_TRUNCATED;
        const int64_t len = ((int64_t)data[pos] << 8) | data[pos + 1];
        if (len < 2) return FD_JPEG_E_MARKER;
        if (pos + len > n) return FD_JPEG_E_TRUNCATED;
        const uint8_t* s = data + pos + 2;                   // payload, `pl` bytes
        const int64_t pl = len - 2;
        pos += len;
        if (m == 0xDB) {                                     // DQT
            int64_t i = 0;
            while (i < pl) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (tq > 3 || pq > 1) return FD_JPEG_E_MARKER;
                const int64_t need = pq ? 128 : 64;
                if (i + 1 + need > pl) return FD_JPEG_E_MARKER;
                int wide = 0;
                for (int k = 0; k < 64; ++k) {
                    const unsigned v = pq ? ((unsigned)s[i + 1 + 2 * k] << 8) | s[i + 2 + 2 * k] : s[i + 1 + k];
                    qtabs[tq][fd_jpeg_natural[k]] = (uint16_t)v;
                    wide |= v > 255u;
                }
                q_defined[tq] = 1;
                q_wide[tq] = (uint8_t)(pq || wide);
                i += 1 + need;
            }
        } else if (m == 0xC4) {                              // DHT
            int64_t i = 0;
            while (i < pl) {
                if (i + 17 > pl) return FD_JPEG_E_MARKER;
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return FD_JPEG_E_MARKER;
                int count = 0;
                for (int k = 0; k < 16; ++k) count += s[i + 1 + k];
                if (count > 256 || i + 17 + count > pl) return FD_JPEG_E_MARKER;
                memcpy(info->huff_bits[tc][th], s + i + 1, 16);
                memset(info->huff_vals[tc][th], 0, 256);
                memcpy(info->huff_vals[tc][th], s + i + 17, (size_t)count);
                info->huff_defined[tc][th] = 1;
                i += 17 + count;
            }
        } else if (m == 0xDD) {                              // DRI
            if (pl != 2) return FD_JPEG_E_MARKER;
            info->restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (pl >= 5 && !memcmp(s, "JFIF", 5)) have_jfif = 1;
        } else if (m == 0xEE) {
            if (pl >= 12 && !memcmp(s, "Adobe", 5)) adobe_transform = s[11];
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {   // a frame header (0xC4 DHT handled above)
            if (have_sof) return FD_JPEG_E_MARKER;
            if (pl < 6) return FD_JPEG_E_MARKER;
            const int precision = s[0], nf = s[5];
            info->height = (s[1] << 8) | s[2];
            info->width = (s[3] << 8) | s[4];
            info->ncomp = nf;
            if (m >= 0xC9) return fd_jpeg_unsupported(info, FD_JPEG_R_ARITHMETIC);
            if (m >= 0xC2) return fd_jpeg_unsupported(info, FD_JPEG_R_PROGRESSIVE);
            if (nf < 1 || pl != 6 + 3 * (int64_t)nf || info->width == 0) return FD_JPEG_E_MARKER;
            if (precision != 8) return fd_jpeg_unsupported(info, FD_JPEG_R_PRECISION);
            if (nf != 1 && nf != 3) return fd_jpeg_unsupported(info, FD_JPEG_R_COMPONENTS);
            if (info->height == 0) return fd_jpeg_unsupported(info, FD_JPEG_R_DNL);
            for (int c = 0; c < nf; ++c) {
                comp_id[c] = s[6 + 3 * c];
                info->h_samp[c] = s[7 + 3 * c] >> 4;
                info->v_samp[c] = s[7 + 3 * c] & 15;
                comp_tq[c] = s[8 + 3 * c];
                if (info->h_samp[c] < 1 || info->h_samp[c] > 4 || info->v_samp[c] < 1 || info->v_samp[c] > 4 || comp_tq[c] > 3) return FD_JPEG_E_MARKER;
            }
            have_sof = 1;
        } else if (m == 0xDA) {                              // SOS: the end of the headers
            if (!have_sof || pl < 1) return FD_JPEG_E_MARKER;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || pl != 4 + 2 * (int64_t)ns) return FD_JPEG_E_MARKER;
            if (ns != info->ncomp) return fd_jpeg_unsupported(info, FD_JPEG_R_MULTISCAN);
            for (int c = 0; c < ns; ++c) {
                int found = -1;
                for (int k = 0; k < info->ncomp; ++k)
                    if (comp_id[k] == s[1 + 2 * c]) { found = k; break; }
                if (found < 0) return FD_JPEG_E_MARKER;
                if (found != c) return fd_jpeg_unsupported(info, FD_JPEG_R_MULTISCAN);   // another interleave order
                info->dc_tab[c] = s[2 + 2 * c] >> 4;
                info->ac_tab[c] = s[2 + 2 * c] & 15;
                if (info->dc_tab[c] > 3 || info->ac_tab[c] > 3) return FD_JPEG_E_MARKER;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return FD_JPEG_E_MARKER;   // Ss, Se, Ah / Al of a sequential scan
            info->scan_offset = pos;
            if (info->ncomp == 3) {
                // libjpeg's colour-space guess: JFIF says YCbCr, else Adobe's transform byte, else the component ids
                int rgb = 0;
                if (have_jfif) rgb = 0;
                else if (adobe_transform >= 0) rgb = adobe_transform == 0;
                else rgb = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
                if (rgb) return fd_jpeg_unsupported(info, FD_JPEG_R_RGB);
                const int hs = info->h_samp[0], vs = info->v_samp[0];
                const int luma_ok = (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
                if (!luma_ok || info->h_samp[1] != 1 || info->v_samp[1] != 1 || info->h_samp[2] != 1 || info->v_samp[2] != 1)
                    return fd_jpeg_unsupported(info, FD_JPEG_R_SAMPLING);
            } else {
                info->h_samp[0] = info->v_samp[0] = 1;       // a single-component scan is not interleaved: one block per MCU
            }
            for (int c = 0; c < info->ncomp; ++c) {
                if (!q_defined[comp_tq[c]] || !info->huff_defined[0][info->dc_tab[c]] || !info->huff_defined[1][info->ac_tab[c]]) return FD_JPEG_E_TABLE;
                if (q_wide[comp_tq[c]]) return fd_jpeg_unsupported(info, FD_JPEG_R_PRECISION);
                memcpy(info->qt[c], qtabs[comp_tq[c]], sizeof(info->qt[c]));
            }
            info->h_max = info->h_samp[0];
            info->v_max = info->v_samp[0];
            info->mcus_x = (info->width + 8 * info->h_max - 1) / (8 * info->h_max);
            info->mcus_y = (info->height + 8 * info->v_max - 1) / (8 * info->v_max);
            int64_t blocks = 0;
            for (int c = 0; c < info->ncomp; ++c) {
                info->bw[c] = info->mcus_x * info->h_samp[c];
                info->bh[c] = info->mcus_y * info->v_samp[c];
                blocks += (int64_t)info->bw[c] * info->bh[c];
            }
            info->coef_bytes = blocks * 64 * (int64_t)sizeof(int16_t);
            info->supported = 1;
            info->reason = FD_JPEG_R_NONE;
            return FD_OK;
        }
        // every other segment (APPn, COM, DAC, DNL before a scan, ...) is skipped
    }
}

// ------------------------------------------------------------------------------ Huffman decoding
struct fd_jpeg_htab {
    uint16_t look[512];    // 9 leading bits -> (length << 8) | symbol, 0: the code is longer than 9 bits (or none)
    int32_t maxcode[17];   // largest code of each length, -1: none
    int32_t valoff[17];    // index of a length's first symbol minus its first code
    const uint8_t* vals;
};

static inline int32_t fd_jpeg_build_htab(const uint8_t* bits, const uint8_t* vals, fd_jpeg_htab* t) {
    memset(t->look, 0, sizeof(t->look));
    t->vals = vals;
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits[l - 1];
        t->valoff[l] = k - code;
        if (code + cnt > (1 << l)) return FD_JPEG_E_HUFFMAN;          // more codes than the length holds
        for (int i = 0; i < cnt; ++i, ++code, ++k) {
            if (k > 255) return FD_JPEG_E_HUFFMAN;
            if (l <= 9) {
                const int first = code << (9 - l), span = 1 << (9 - l);
                for (int j = 0; j < span; ++j) t->look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t->maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    return FD_OK;
}

struct fd_jpeg_bits {
    const uint8_t* data;
    int64_t n, pos;
    uint64_t acc;      // the low `nbits` bits are unread, oldest on top
    int nbits;
    int fake;          // zero bits appended after the data ran out (a marker or the end of the stream): always the youngest
    int stopped;
};

static inline void fd_jpeg_fill(fd_jpeg_bits* b) {
    while (b->nbits <= 56) {
        unsigned byte = 0;
        if (!b->stopped) {
            if (b->pos < b->n) {
                byte = b->data[b->pos];
                if (byte == 0xFF) {
                    if (b->pos + 1 < b->n && b->data[b->pos + 1] == 0x00) b->pos += 2;     // a stuffed 0xFF
                    else { b->stopped = 1; byte = 0; }                                        // a marker, or the stream ends inside one
                } else {
                    b->pos += 1;
                }
            } else {
                b->stopped = 1;
            }
        }
        if (b->stopped) b->fake += 8;
        b->acc = (b->acc << 8) | byte;
        b->nbits += 8;
    }
}

static inline unsigned fd_jpeg_get(fd_jpeg_bits* b, int s) {      // 1 <= s <= 16
    if (b->nbits < s) fd_jpeg_fill(b);
    b->nbits -= s;
    return (unsigned)(b->acc >> b->nbits) & ((1u << s) - 1u);
}

static inline int fd_jpeg_symbol(fd_jpeg_bits* b, const fd_jpeg_htab* t) {   // -1: no code matches
    if (b->nbits < 16) fd_jpeg_fill(b);
    const unsigned e = t->look[(b->acc >> (b->nbits - 9)) & 511u];
    if (e) {
        b->nbits -= (int)(e >> 8);
        return (int)(e & 255u);
    }
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)((b->acc >> (b->nbits - l)) & ((1u << l) - 1u));
        if (code <= t->maxcode[l]) {
            const int32_t idx = t->valoff[l] + code;
            if (idx < 0 || idx > 255) return -1;
            b->nbits -= l;
            return t->vals[idx];
        }
    }
    return -1;
}

// what went wrong first: a code read from bits the stream does not hold is the stream's end, not a bad code
#define FD_JPEG_FAIL(b, code) ((b).fake > (b).nbits ? FD_JPEG_E_TRUNCATED : (code))

static inline int32_t fd_jpeg_extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v; }

extern "C" FD_JPEG_API int32_t fd_jpeg_entropy_decode(const uint8_t* data, int64_t n, const fd_jpeg_info* info, int16_t* coefs, int64_t coef_bytes) {
    if (!data || !info || !coefs || n < 0) return FD_JPEG_E_BUFFER;
    if (!info->supported) return FD_JPEG_E_UNSUPPORTED;
    // the block grid is re-derived from the header fields: nothing below trusts a size it did not check
    const int nc = info->ncomp;
    if (nc != 1 && nc != 3) return FD_JPEG_E_UNSUPPORTED;
    if (info->width < 1 || info->width > 65535 || info->height < 1 || info->height > 65535) return FD_JPEG_E_MARKER;
    if (info->scan_offset < 0 || info->scan_offset > n || info->restart_interval < 0) return FD_JPEG_E_MARKER;
    const int hmax = info->h_samp[0], vmax = info->v_samp[0];
    if (hmax < 1 || hmax > 2 || vmax < 1 || vmax > 2) return FD_JPEG_E_UNSUPPORTED;
    const int32_t mcus_x = (info->width + 8 * hmax - 1) / (8 * hmax), mcus_y = (info->height + 8 * vmax - 1) / (8 * vmax);
    int64_t base[FD_JPEG_MAX_COMP], blocks = 0;
    int32_t bw[FD_JPEG_MAX_COMP];
    fd_jpeg_htab tabs[2][4];
    uint8_t built[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int c = 0; c < nc; ++c) {
        const int hs = info->h_samp[c], vs = info->v_samp[c];
        if (hs < 1 || hs > hmax || vs < 1 || vs > vmax || (c > 0 && (hs != 1 || vs != 1))) return FD_JPEG_E_UNSUPPORTED;
        base[c] = blocks * 64;
        bw[c] = mcus_x * hs;
        blocks += (int64_t)bw[c] * (mcus_y * vs);
        const int td = info->dc_tab[c], ta = info->ac_tab[c];
        if (td < 0 || td > 3 || ta < 0 || ta > 3 || !info->huff_defined[0][td] || !info->huff_defined[1][ta]) return FD_JPEG_E_TABLE;
        if (!built[0][td]) {
            if (fd_jpeg_build_htab(info->huff_bits[0][td], info->huff_vals[0][td], &tabs[0][td]) != FD_OK) return FD_JPEG_E_HUFFMAN;
            built[0][td] = 1;
        }
        if (!built[1][ta]) {
            if (fd_jpeg_build_htab(info->huff_bits[1][ta], info->huff_vals[1][ta], &tabs[1][ta]) != FD_OK) return FD_JPEG_E_HUFFMAN;
            built[1][ta] = 1;
        }
    }
    const int64_t need = blocks * 64 * (int64_t)sizeof(int16_t);
    if (need != info->coef_bytes || coef_bytes < need) return FD_JPEG_E_BUFFER;
    memset(coefs, 0, (size_t)need);

    fd_jpeg_bits b = {data, n, info->scan_offset, 0, 0, 0, 0};
    int32_t pred[FD_JPEG_MAX_COMP] = {0, 0, 0};
    const int32_t ri = info->restart_interval;
    int64_t mcu = 0;
    for (int32_t my = 0; my < mcus_y; ++my) {
        for (int32_t mx = 0; mx < mcus_x; ++mx, ++mcu) {
            if (ri && mcu && mcu % ri == 0) {
                // RSTn: drop the rest of the current byte (and whatever pads the interval), find the marker, start afresh
                const unsigned want = 0xD0u + (unsigned)((mcu / ri - 1) & 7);
                int64_t p = b.pos;
                for (;;) {
                    if (p + 1 >= n) return FD_JPEG_E_TRUNCATED;
                    if (data[p] != 0xFF) { ++p; continue; }
                    const unsigned m = data[p + 1];
                    if (m == 0xFF) { ++p; continue; }
                    if (m == 0x00) { p += 2; continue; }
                    if (m != want) return FD_JPEG_E_MARKER;
                    p += 2;
                    break;
                }
                b.pos = p;
                b.acc = 0;
                b.nbits = b.fake = b.stopped = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c) {
                const fd_jpeg_htab* dc = &tabs[0][info->dc_tab[c]];
                const fd_jpeg_htab* ac = &tabs[1][info->ac_tab[c]];
                const int hs = info->h_samp[c], vs = info->v_samp[c];
                for (int v = 0; v < vs; ++v) {
                    for (int h = 0; h < hs; ++h) {
                        const int64_t blk = (int64_t)(my * vs + v) * bw[c] + (mx * hs + h);
                        int16_t* out = coefs + base[c] + blk * 64;          // blk < bw * bh of the component: inside `need`
                        int s = fd_jpeg_symbol(&b, dc);
                        if (s < 0 || s > 15) return FD_JPEG_FAIL(b, FD_JPEG_E_HUFFMAN);
                        if (s) pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)fd_jpeg_extend(fd_jpeg_get(&b, s), s));
                        out[0] = (int16_t)(uint16_t)(uint32_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = fd_jpeg_symbol(&b, ac);
                            if (rs < 0) return FD_JPEG_FAIL(b, FD_JPEG_E_HUFFMAN);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s) {
                                k += r;
                                if (k > 63) return FD_JPEG_FAIL(b, FD_JPEG_E_COEF_INDEX);
                                out[fd_jpeg_natural[k]] = (int16_t)fd_jpeg_extend(fd_jpeg_get(&b, s), s);
                                ++k;
                            } else if (r == 15) {
                                k += 16;
                            } else {
                                break;
                            }
                        }
                        if (b.fake > b.nbits) return FD_JPEG_E_TRUNCATED;   // the block used bits the stream does not hold
                    }
                }
            }
        }
    }
    return FD_OK;
}
