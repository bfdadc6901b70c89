// form_probe.cpp - prints what csrc/dc_form.h decides for the cases on stdin, one JSON line per case (tests/test_host_form.py, _known,
// _guided, _takes, through helpers.form_probe).  A case is a command (form | plan | tail | spg) followed by key=value pairs;
// env=NAME,NAME sets those environment switches while Switches::read() runs.  B is the internal batch as given; without it the batch is
// musics x takes (x 2 when guided) clips.  `plan` prints the LoopPlan of a loop of S steps (flags, tail_split, override, profile,
// no_graph) and, with step=i, the options of step i of its part part=k.  A case with magic_period=p magic_takes=k instead checks
// film_magic(p, k p) against g / p for every g < k p.  Host only: c++ -std=c++17 -I <package>/csrc.
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
        // a finalized 8-layer sampler on a device (pack_model / upload_model, dc_api.hip)
        Settings s;
        s.precision = num("prec", DCF_FP16), s.fmt.set_precision(s.precision), s.no_eff = num("no_eff", 0), s.clip_aligned = num("clip_aligned", -1);
        s.l16_own = num("l16_own", 0), s.num_layers = 8, s.split_model = num("split_model", 1), s.film_w16 = true;
        s.film_w16_tail = s.precision == DCF_BF16, s.l16_max_units = 32;
        const std::optional<int> override_tail = a.count("override") ? std::optional<int>(num("override", 0)) : std::nullopt;
        if (cmd == "tail") {
            const LoopTail t = loop_tail(s, num("tail_split", -1), override_tail, num("flags", 0), num("Tx", 1800), num("S", 50));
            printf("{\"tail\": %d, \"tail_all\": %d}\n", t.tail, (int)t.tail_all);
            continue;
        }
        const int takes = num("takes", 1), guided = num("guided", 0);
        const int B = num("B", num("musics", 1) * takes * (guided ? 2 : 1)), Tx = num("Tx", 1800), ncu = num("num_cu", 256);
        const int T = clip_stride(s, w, B, Tx, ncu), G = (B * T + 31) / 32;        // (ensure_workspace, dc_api.hip)
        const Geometry geo{B, T, Tx, G, ncu, rec_capacity((size_t)G)};
        StepOpts o;
        if (cmd == "plan") {
            LoopOpts lo;
            lo.S = num("S", 50), lo.flags = num("flags", 0), lo.guided = guided, lo.takes = takes, lo.profile = num("profile", 0);
            lo.no_graph = num("no_graph", 0), lo.tail_split = num("tail_split", -1), lo.env_tail = override_tail;
            const LoopPlan p = loop_plan(geo, s, w, lo);
            if (!a.count("step")) {
                printf("{\"g1_loop\": %d, \"eager\": %d, \"parts\": [", (int)p.g1_loop, (int)p.eager);
                for (size_t k = 0; k < p.parts.size(); ++k) {
                    const LoopPart& q = p.parts[k];
                    const auto& [kB, kT, kTx, kK, kbits, kperiod] = q.key;
                    printf("%s{\"steps\": %d, \"split_n\": %d, \"launches\": %d, \"key\": [%d, %d, %d, %d, %llu, %d]}", k ? ", " : "", q.steps, q.split_n,
                           q.launches, kB, kT, kTx, kK, kbits, kperiod);
                }
                printf("]}\n");
                continue;
            }
            o = loop_step(p, p.parts.at(num("part", 0)), lo, num("step", 0));
            printf("{\"loop_mode\": %d, \"graph_step\": %d, \"split\": %d, \"g1_loop\": %d, \"next_plain\": %d, \"embedded\": %d, \"profile\": %d, "
                   "\"known\": %d, \"guided\": %d, \"takes\": %d}\n", (int)o.loop_mode, o.graph_step, (int)o.split, (int)o.g1_loop, (int)o.next_plain,
                   (int)o.embedded, (int)o.profile, (int)o.known, (int)o.guided, o.takes);
            continue;
        }
        o.loop_mode = num("loop", 0), o.graph_step = num("graph_step", -1), o.split = num("split", 0), o.g1_loop = num("g1_loop", 0);
        o.next_plain = num("next_plain", 0), o.embedded = num("embedded", 0), o.profile = num("profile", 0), o.known = num("known", 0);
        o.guided = guided, o.takes = takes;
        o.dbg = Hooks{num("layers", -1), num("stage", 0), num("first", -1)};
        const StepForm f = step_form(geo, s, w, o, num("stamps", 0) != 0);
        const FilmShare sh = film_share(B, T, G, guided, takes, f.fuse_silu, w);
        printf("{\"B\": %d, \"stride\": %d, \"G\": %d, \"error\": \"%s\", \"bits\": %llu, \"switch_bits\": %llu, \"key_bits\": %llu, \"key_period\": %d", B, T,
               G, f.error.c_str(), w.bits(), w.bits(), guided_key_bits(f.guided, f.shared_film), takes_key_period(sh));
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
