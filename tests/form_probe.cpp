// form_probe.cpp - prints what csrc/dc_form.h decides for the cases on stdin, one JSON line per case (tests/test_host_form.py).
// A case is a command (form | tail | spg) followed by key=value pairs; env=NAME,NAME sets those environment switches while
// Switches::read() runs.  Host only: c++ -std=c++17 -I <package>/csrc.
#include <iostream>
#include <map>
#include <sstream>
#include <vector>

#include "dc_form.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, kv;
        std::map<std::string, std::string> a;
        in >> cmd;
        while (in >> kv) a[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
        const auto num = [&](const char* k, int dflt) { return a.count(k) ? atoi(a[k].c_str()) : dflt; };
        if (cmd == "spg") {
            printf("{\"steps_per_graph\": %d}\n", steps_per_graph(num("S", 1)));
            continue;
        }
        std::vector<std::string> env;
        std::istringstream names(a["env"]);
        for (std::string n; std::getline(names, n, ',');) env.push_back(n);
        for (const auto& n : env) setenv(n.c_str(), "1", 1);
        const Switches w = Switches::read();
        for (const auto& n : env) unsetenv(n.c_str());
        // a finalized 8-layer sampler on a device (pack_model / upload_model, dc_api.hip)
        Settings s;
        s.precision = num("prec", DCF_FP16), s.fmt.set_precision(s.precision), s.no_eff = num("no_eff", 0), s.clip_aligned = num("clip_aligned", -1);
        s.l16_own = num("l16_own", 0), s.num_layers = 8, s.split_model = num("split_model", 1), s.film_w16 = true;
        s.film_w16_tail = s.precision == DCF_BF16, s.l16_max_units = 32;
        if (cmd == "tail") {
            const LoopTail t = loop_tail(s, num("tail_split", -1), a.count("override") ? std::optional<int>(num("override", 0)) : std::nullopt,
                                         num("flags", 0), num("Tx", 1800), num("S", 50));
            printf("{\"tail\": %d, \"tail_all\": %d}\n", t.tail, (int)t.tail_all);
            continue;
        }
        const int B = num("B", 1), Tx = num("Tx", 1800), ncu = num("num_cu", 256);
        const int T = clip_stride(s, w, B, Tx, ncu), G = (B * T + 31) / 32;        // (ensure_workspace, dc_api.hip)
        StepOpts o;
        o.loop_mode = num("loop", 0), o.graph_step = num("graph_step", -1), o.split = num("split", 0), o.g1_loop = num("g1_loop", 0);
        o.next_plain = num("next_plain", 0), o.embedded = num("embedded", 0), o.profile = num("profile", 0);
        o.dbg = Hooks{num("layers", -1), num("stage", 0), num("first", -1)};
        const StepForm f = step_form(Geometry{B, T, Tx, G, ncu, rec_capacity((size_t)G)}, s, w, o, num("stamps", 0) != 0);
        printf("{\"stride\": %d, \"bits\": %llu, \"error\": \"%s\"", T, w.bits(), f.error.c_str());
#define FIELD(n) printf(", \"" #n "\": %lld", (long long)f.n);
        FIELD(ss) FIELD(film_tail) FIELD(fs) FIELD(ff) FIELD(fuse_silu) FIELD(folded) FIELD(adapt) FIELD(wgr) FIELD(narrow) FIELD(aligned)
        FIELD(layer16) FIELD(l16_shared) FIELD(upc) FIELD(upc16) FIELD(upc_narrow) FIELD(nwg) FIELD(rec_stride) FIELD(mixed_form)
        FIELD(embed_next) FIELD(fuse_embed) FIELD(fuse_extra) FIELD(g1_tiles) FIELD(upd_flags) FIELD(nl_run) FIELD(stop_stage)
        printf("}\n");
    }
    return 0;
}
