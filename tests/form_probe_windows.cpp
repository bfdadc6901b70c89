// form_probe_windows.cpp - form_probe.cpp's `form` and `plan` commands with the windows option of csrc/dc_form.h (StepOpts::windows,
// LoopOpts::windows / win_L; tests/test_host_windows.py through helpers_windows.windows_probe).  A case is a command followed by
// key=value pairs; B is the INTERNAL batch (W windows x the pieces, x 2 when guided); windows=W (0: none) and win_L=L describe the plan;
// env=NAME,NAME sets those environment switches while Switches::read() runs.  One JSON line per case.  Host only:
// c++ -std=c++17 -I <package>/csrc.
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
        std::vector<std::string> env;
        std::istringstream names(a["env"]);
        for (std::string n; std::getline(names, n, ',');) env.push_back(n);
        for (const auto& n : env) setenv(n.c_str(), "1", 1);
        const Switches w = Switches::read();
        for (const auto& n : env) unsetenv(n.c_str());
        // a finalized 8-layer sampler on a device, as form_probe.cpp builds it
        Settings s;
        s.precision = num("prec", DCF_FP16), s.fmt.set_precision(s.precision), s.no_eff = num("no_eff", 0), s.clip_aligned = num("clip_aligned", -1);
        s.l16_own = num("l16_own", 0), s.num_layers = 8, s.split_model = num("split_model", 1), s.film_w16 = true;
        s.film_w16_tail = s.precision == DCF_BF16, s.l16_max_units = 32;
        const int takes = num("takes", 1), guided = num("guided", 0), windows = num("windows", 0), win_L = num("win_L", 0);
        const int B = num("B", 1), Tx = num("Tx", 1800), ncu = num("num_cu", 256);
        const int T = clip_stride(s, w, B, Tx, ncu), G = (B * T + 31) / 32;
        const Geometry geo{B, T, Tx, G, ncu, rec_capacity((size_t)G)};
        if (cmd == "plan") {
            LoopOpts lo;
            lo.S = num("S", 50), lo.flags = num("flags", 0), lo.guided = guided, lo.takes = takes, lo.windows = windows, lo.win_L = win_L;
            lo.profile = num("profile", 0), lo.no_graph = num("no_graph", 0), lo.tail_split = num("tail_split", -1);
            const LoopPlan p = loop_plan(geo, s, w, lo);
            const StepOpts o = loop_step(p, p.parts.at(0), lo, 0);
            printf("{\"eager\": %d, \"step_windows\": %d, \"parts\": [", (int)p.eager, (int)o.windows);
            for (size_t k = 0; k < p.parts.size(); ++k) {
                const LoopPart& q = p.parts[k];
                const auto& [kB, kT, kTx, kK, kbits, klast] = q.key;
                printf("%s{\"steps\": %d, \"split_n\": %d, \"launches\": %d, \"key\": [%d, %d, %d, %d, %llu, %d]}", k ? ", " : "", q.steps, q.split_n,
                       q.launches, kB, kT, kTx, kK, kbits, klast);
            }
            printf("]}\n");
            continue;
        }
        StepOpts o;
        o.loop_mode = num("loop", 0), o.graph_step = num("graph_step", -1), o.split = num("split", 0), o.g1_loop = num("g1_loop", 0);
        o.next_plain = num("next_plain", 0), o.embedded = num("embedded", 0), o.profile = num("profile", 0), o.known = num("known", 0);
        o.guided = guided, o.takes = takes, o.windows = windows > 0;
        o.dbg = Hooks{num("layers", -1), num("stage", 0), num("first", -1)};
        const StepForm f = step_form(geo, s, w, o, num("stamps", 0) != 0);
        printf("{\"B\": %d, \"stride\": %d, \"G\": %d, \"error\": \"%s\", \"switch_bits\": %llu, \"key_bits\": %llu", B, T, G, f.error.c_str(), w.bits(),
               guided_key_bits(f.guided, f.shared_film) | windows_key_bits(windows));
#define FIELD(n) printf(", \"" #n "\": %lld", (long long)f.n);
        FIELD(ss) FIELD(film_tail) FIELD(fs) FIELD(ff) FIELD(fuse_silu) FIELD(folded) FIELD(adapt) FIELD(wgr) FIELD(narrow) FIELD(aligned)
        FIELD(layer16) FIELD(l16_shared) FIELD(upc) FIELD(upc16) FIELD(upc_narrow) FIELD(nwg) FIELD(rec_stride) FIELD(mixed_form)
        FIELD(embed_next) FIELD(fuse_embed) FIELD(fuse_extra) FIELD(g1_tiles) FIELD(upd_flags) FIELD(nl_run) FIELD(stop_stage)
        FIELD(guided) FIELD(windows) FIELD(shared_film) FIELD(film_groups) FIELD(film_period) FIELD(film_wrap)
        printf("}\n");
    }
    return 0;
}
