// tests/abi/jpeg_host_check.cpp — the host half of the JPEG decoder (csrc/fd_jpeg_host.h) under the host sanitizers, on its own:
// no Python, no HIP, no GPU.  tests/test_jpeg_host_asan_cpu.py builds it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/abi/jpeg_host_check.cpp -o ...
// and runs it on stream files written from tests/golden/g16_jpeg.npz:  jpeg_host_check FILE...
// Per file: fd_jpeg_parse + fd_jpeg_entropy_decode over every prefix, and over 2 000 deterministic mutations (one byte replaced, or
// one bit flipped).  Every input and output lives in an exactly sized heap block, so a read past `n` or a write past `coef_bytes` is
// the sanitizer's to report.  The program itself returns non-zero only on an inconsistency: a prefix shorter than the headers that
// parses, or a byte behind the coefficients' end that changed.
#include "../../pytorch_object_detection_amd/csrc/fd_jpeg_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long g_ok = 0, g_unsupported = 0, g_errors = 0, g_failures = 0;

// One parse + decode of exactly n bytes (copied into a block of n bytes).  Returns fd_jpeg_parse's code.
static int32_t run_once(const uint8_t* bytes, int64_t n) {
    uint8_t* data = (uint8_t*)malloc(n ? (size_t)n : 1);
    if (n) memcpy(data, bytes, (size_t)n);
    fd_jpeg_info info;
    const int32_t rc = fd_jpeg_parse(data, n, &info);
    if (rc != FD_OK) {
        ++g_errors;
    } else if (!info.supported) {
        ++g_unsupported;
    } else if (info.coef_bytes > (64ll << 20)) {
        ++g_unsupported;                                      // a mutated size: not worth the memory here
    } else {
        const size_t guard = 64, cb = (size_t)info.coef_bytes;
        uint8_t* coefs = (uint8_t*)malloc(cb + guard);        // 16-byte aligned: fine for int16
        memset(coefs + cb, 0xC3, guard);
        const int32_t rd = fd_jpeg_entropy_decode(data, n, &info, (int16_t*)coefs, (int64_t)cb);
        if (rd == FD_OK) ++g_ok; else ++g_errors;
        for (size_t i = 0; i < guard; ++i)
            if (coefs[cb + i] != 0xC3) {
                fprintf(stderr, "jpeg_host_check: byte %zu behind coef_bytes = %zu was written (n = %lld)\n", i, cb, (long long)n);
                ++g_failures;
                break;
            }
        if (cb >= 2 && fd_jpeg_entropy_decode(data, n, &info, (int16_t*)coefs, (int64_t)cb - 2) != FD_JPEG_E_BUFFER) {
            fprintf(stderr, "jpeg_host_check: a buffer two bytes short was not refused\n");
            ++g_failures;
        }
        free(coefs);
    }
    free(data);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_host_check FILE...\n");
        return 2;
    }
    long prefixes = 0, mutations = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "jpeg_host_check: cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> s;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) s.insert(s.end(), chunk, chunk + got);
        fclose(f);
        const int64_t n = (int64_t)s.size();
        fd_jpeg_info whole;
        if (fd_jpeg_parse(s.data(), n, &whole) != FD_OK || !whole.supported) { fprintf(stderr, "jpeg_host_check: %s is not a supported stream\n", argv[a]); return 2; }
        for (int64_t k = 0; k <= n; ++k, ++prefixes) {
            const int32_t rc = run_once(s.data(), k);
            if (k < whole.scan_offset && rc == FD_OK) {
                fprintf(stderr, "jpeg_host_check: %s: the %lld-byte prefix parsed, the headers are %lld bytes long\n", argv[a], (long long)k, (long long)whole.scan_offset);
                ++g_failures;
            }
        }
        uint32_t x = 0x9E3779B9u ^ (uint32_t)n;               // xorshift32: the same mutations in every run
        std::vector<uint8_t> m(s);
        for (int k = 0; k < 2000; ++k, ++mutations) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            const size_t at = (size_t)(x % (uint32_t)n);
            const uint8_t old = m[at];
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            m[at] = (k & 1) ? (uint8_t)(old ^ (1u << (x & 7))) : (uint8_t)(x >> 8);
            run_once(m.data(), n);
            m[at] = old;
        }
    }
    printf("jpeg_host_check: %d streams, %ld prefixes, %ld mutations: %ld decoded, %ld unsupported, %ld error codes, %ld inconsistencies\n", argc - 1, prefixes, mutations,
           g_ok, g_unsupported, g_errors, g_failures);
    return g_failures ? 1 : 0;
}
