// Host probe of the M2SNet fuse head's packing (csrc/dc_pack.h, m2s_head_pack), for tests/test_host_m2snet.py: reads the six
// fuse_layer tensors (fp32, in state_dict order) from argv[1], writes the device image the library would upload to argv[2].
#include <cstdio>

#include "dc_pack.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const struct {
        const char* name;
        size_t numel;
    } spec[6] = {{"fuse_layer.0.weight", 64 * 128}, {"fuse_layer.0.bias", 64}, {"fuse_layer.2.weight", 64 * 64},
                 {"fuse_layer.2.bias", 64},         {"fuse_layer.4.weight", 64}, {"fuse_layer.4.bias", 1}};
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    DcParams params;
    for (const auto& s : spec) {
        std::vector<float> v(s.numel);
        if (fread(v.data(), sizeof(float), s.numel, f) != s.numel) return 4;
        params[s.name] = v;
    }
    fclose(f);
    const std::vector<float> img = m2s_head_pack(params);
    if ((int)img.size() != kHeadFloats) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(img.data(), sizeof(float), img.size(), o) != img.size()) return 6;
    fclose(o);
    printf("%d %d %d %d %d %d %d\n", kHeadW0, kHeadB0, kHeadW1, kHeadB1, kHeadW2, kHeadB2, kHeadFloats);
    return 0;
}
