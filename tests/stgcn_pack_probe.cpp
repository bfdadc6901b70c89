// Host probe of the ST-GCN motion encoder's folding and packing (csrc/dc_pack.h, stgcn_pack), for tests/test_motion_metrics_host.py.
// `probe list` prints "name numel" for every entry of stgcn_required() and of stgcn_ignored(), the latter marked "ignored";
// `probe in out` reads the required tensors (fp32, in that order) from `in`, writes the device image the library would upload to
// `out` and prints the layout constants.
#include <cstdio>
#include <cstring>

#include "dc_pack.h"

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "list")) {
        for (const auto& r : stgcn_required()) printf("%s %zu\n", r.first.c_str(), r.second);
        for (const auto& r : stgcn_ignored()) printf("%s %zu ignored\n", r.first.c_str(), r.second);
        return 0;
    }
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    DcParams params;
    for (const auto& r : stgcn_required()) {
        std::vector<float> v(r.second);
        if (fread(v.data(), sizeof(float), r.second, f) != r.second) return 4;
        params[r.first] = v;
    }
    fclose(f);
    const std::vector<float> img = stgcn_pack(params);
    if ((int)img.size() != kStgcnFloats) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(img.data(), sizeof(float), img.size(), o) != img.size()) return 6;
    fclose(o);
    printf("%d %d %d %d %d %d %d %d %d %d\n", kStgcnW1, kStgcnW2, kStgcnB1, kStgcnB2, kStgcnAhat, kStgcnBlockFloats, kStgcnDbn, kStgcnFcW,
           kStgcnFcB, kStgcnFloats);
    return 0;
}
