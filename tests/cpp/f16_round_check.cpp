// Stand-alone check of host/uspmv_f16_round.hpp, the text the device-side partition compiles for gfx950: reads 64-bit patterns, writes the
// binary16 bits uspmv_f64_bits_to_f16 gives for each and the bits of the double uspmv_f16_to_f64_bits widens them to.
// tests/test_ap_device_setup_api.py compares both files with numpy, bit for bit.
//   f16_round_check <in: uint64 patterns> <out: uint16 halves> <out: uint64 widened>
#include <cstdio>
#include <vector>

#include "uspmv_f16_round.hpp"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> in(n), wide(n);
    std::vector<uint16_t> half(n);
    if (fread(in.data(), 8, n, f) != n) return 4;
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        half[i] = uspmv_f64_bits_to_f16(in[i]);
        wide[i] = uspmv_f16_to_f64_bits(half[i]);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(half.data(), 2, n, f) != n) return 5;
    fclose(f);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(wide.data(), 8, n, f) != n) return 6;
    fclose(f);
    printf("%zu OK\n", n);
    return 0;
}
