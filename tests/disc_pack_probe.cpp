// Host probe of the M2S-GAN critic's packing and of the Welch window-and-twiddle table (csrc/dc_pack.h: disc_required, disc_pack,
// welch_table), for tests/test_host_rhythm.py.
// `probe list` prints "name numel" for every entry of disc_required(); `probe table out` writes welch_table() (fp32 [64][256]) to
// `out`; `probe in out` reads the required tensors (fp32, in that order) from `in`, writes the device image the library would
// upload to `out` and prints its offsets: w0 b0 w1 b1 w2 b2 fw0 fb0 fw1 fb1 fw2 fb2 floats.
#include <cstdio>
#include <cstring>

#include "dc_pack.h"

static int dump(const char* path, const std::vector<float>& v) {
    FILE* o = fopen(path, "wb");
    if (!o || fwrite(v.data(), sizeof(float), v.size(), o) != v.size()) return 6;
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "list")) {
        for (const auto& r : disc_required()) printf("%s %zu\n", r.first.c_str(), r.second);
        return 0;
    }
    if (argc != 3) return 2;
    if (!strcmp(argv[1], "table")) return dump(argv[2], welch_table());
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    DcParams params;
    for (const auto& r : disc_required()) {
        std::vector<float> v(r.second);
        if (fread(v.data(), sizeof(float), r.second, f) != r.second) return 4;
        params[r.first] = v;
    }
    fclose(f);
    const DiscImage I = disc_pack(params);
    if (const int rc = dump(argv[2], I.img)) return rc;
    for (int i = 0; i < kDiscStages; ++i) printf("%zu %zu ", I.w[i], I.b[i]);
    for (int i = 0; i < 3; ++i) printf("%zu %zu ", I.fw[i], I.fb[i]);
    printf("%zu\n", I.img.size());
    return 0;
}
