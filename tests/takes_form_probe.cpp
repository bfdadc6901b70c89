// takes_form_probe.cpp - prints what csrc/dc_form.h decides for a loop step over several takes per music (tests/test_host_takes.py;
// the wider rule has its own probe, form_probe.cpp, guidance guided_form_probe.cpp).  A case on stdin is key=value pairs: musics (the
// CALLER's B) takes guided Tx prec no_eff graph_step next_plain split g1_loop known profile num_cu env=NAME,NAME; the internal batch is
// musics x takes (x 2 when guided) clips.  A case "magic_period=p magic_takes=k" instead checks film_magic(p, k p) against g / p for every
// g < k p.  One JSON line per case.  Host only: c++ -std=c++17 -I <package>/csrc.
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
        if (a.count("magic_period")) {      // the kernels' quotient, (g m) >> 32 (film_tile_group, dc_dev.h), against g / p
            const long long p = num("magic_period", 2), wrap = p * num("magic_takes", 2);
            const unsigned m = film_magic((int)p, (int)wrap);
            long long wrong = 0;
            for (long long g = 0; g < wrap; ++g) wrong += (unsigned)(((unsigned long long)g * m) >> 32) != (unsigned)(g / p);
            printf("{\"magic\": %u, \"checked\": %lld, \"wrong\": %lld, \"unshared\": %u}\n", m, wrap, wrong, film_magic((int)wrap, (int)wrap));
            continue;
        }
        std::vector<std::string> env;
        std::istringstream names(a["env"]);
        for (std::string n; std::getline(names, n, ',');) env.push_back(n);
        for (const auto& n : env) setenv(n.c_str(), "1", 1);
        const Switches w = Switches::read();
        for (const auto& n : env) unsetenv(n.c_str());
        Settings s;      // a finalized 8-layer sampler on a device
        s.precision = num("prec", DCF_FP16), s.fmt.set_precision(s.precision), s.no_eff = num("no_eff", 0);
        s.num_layers = 8, s.split_model = true, s.film_w16 = true, s.film_w16_tail = s.precision == DCF_BF16, s.l16_max_units = 32;
        const int musics = num("musics", 1), takes = num("takes", 1), guided = num("guided", 0);
        const int B = musics * takes * (guided ? 2 : 1), Tx = num("Tx", 1800), ncu = num("num_cu", 256);
        const int T = clip_stride(s, w, B, Tx, ncu), G = (B * T + 31) / 32;
        StepOpts o;
        o.loop_mode = true, o.graph_step = num("graph_step", 0), o.split = num("split", 0), o.g1_loop = num("g1_loop", 1);
        o.next_plain = num("next_plain", 1), o.known = num("known", 0), o.guided = guided, o.profile = num("profile", 0);
        o.embedded = num("embedded", 0);
        o.takes = takes;
        const StepForm f = step_form(Geometry{B, T, Tx, G, ncu, rec_capacity((size_t)G)}, s, w, o, false);
        const FilmShare sh = film_share(B, T, G, guided, takes, f.fuse_silu, w);
        printf("{\"B\": %d, \"stride\": %d, \"G\": %d, \"error\": \"%s\", \"switch_bits\": %llu, \"key_bits\": %llu, \"key_period\": %d", B, T, G,
               f.error.c_str(), w.bits(), guided_key_bits(f.guided, f.shared_film), takes_key_period(sh));
        printf(", \"share_period\": %d, \"share_wrap\": %d, \"share_groups\": %d", sh.period, sh.wrap, sh.groups);
#define FIELD(n) printf(", \"" #n "\": %lld", (long long)f.n);
        FIELD(ss) FIELD(film_tail) FIELD(fs) FIELD(ff) FIELD(fuse_silu) FIELD(folded) FIELD(adapt) FIELD(wgr) FIELD(narrow) FIELD(aligned)
        FIELD(layer16) FIELD(l16_shared) FIELD(upc) FIELD(upc16) FIELD(upc_narrow) FIELD(nwg) FIELD(rec_stride) FIELD(mixed_form)
        FIELD(embed_next) FIELD(fuse_embed) FIELD(fuse_extra) FIELD(g1_tiles) FIELD(upd_flags) FIELD(nl_run) FIELD(stop_stage)
        FIELD(guided) FIELD(shared_film) FIELD(film_groups) FIELD(film_period) FIELD(film_wrap)
        printf("}\n");
    }
    return 0;
}
