// idle_form_probe.cpp - what csrc/dc_form.h decides about the padding waves' barrier-only path (Settings::idle_wave_path ->
// StepForm::idle_path, bit 29 of a captured graph's key) for the cases on stdin, one JSON line per case (tests/test_host_idle_waves.py).
// A case is key=value pairs: idle (the setting, default 1), B, Tx, prec, split, layers, stage, stamps, no_eff, env=NAME,NAME.
// Host only: c++ -std=c++17 -I <package>/csrc.
#include <iostream>
#include <map>
#include <sstream>
#include <vector>

#include "dc_form.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kv;
        std::map<std::string, std::string> a;
        while (in >> kv) a[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
        const auto num = [&](const char* k, int dflt) { return a.count(k) ? atoi(a[k].c_str()) : dflt; };
        std::vector<std::string> env;
        std::istringstream names(a["env"]);
        for (std::string n; std::getline(names, n, ',');) env.push_back(n);
        for (const auto& n : env) setenv(n.c_str(), "1", 1);
        const Switches w = Switches::read();
        for (const auto& n : env) unsetenv(n.c_str());
        Settings s;      // a finalized 8-layer sampler on a device
        const bool dflt_on = s.idle_wave_path;
        s.precision = num("prec", DCF_FP16), s.fmt.set_precision(s.precision), s.no_eff = num("no_eff", 0), s.num_layers = 8;
        s.split_model = true, s.film_w16 = true, s.film_w16_tail = s.precision == DCF_BF16, s.l16_max_units = 32;
        s.idle_wave_path = num("idle", 1) != 0;
        const int B = num("B", 32), Tx = num("Tx", 1800), ncu = 256;
        const int T = clip_stride(s, w, B, Tx, ncu), G = (B * T + 31) / 32;
        const Geometry geo{B, T, Tx, G, ncu, rec_capacity((size_t)G)};
        StepOpts o;
        o.loop_mode = true, o.graph_step = 0, o.g1_loop = true, o.next_plain = true, o.split = num("split", 0);
        o.dbg = Hooks{num("layers", -1), num("stage", 0), -1};
        if (!o.dbg.production()) o.loop_mode = false, o.graph_step = -1, o.next_plain = false;
        const StepForm f = step_form(geo, s, w, o, num("stamps", 0) != 0);
        LoopOpts lo;
        lo.S = 50;
        const LoopPlan p = loop_plan(geo, s, w, lo);
        printf("{\"default_on\": %d, \"error\": \"%s\", \"idle_path\": %d, \"wgr\": %d, \"narrow\": %d, \"ss\": %d, \"aligned\": %d, \"upc\": %d, \"key_bits\": %llu}\n",
               (int)dflt_on, f.error.c_str(), (int)f.idle_path, (int)f.wgr, (int)f.narrow, (int)f.ss, (int)f.aligned, f.upc,
               std::get<4>(p.parts.at(0).key));
    }
    return 0;
}
