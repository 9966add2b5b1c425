// The planner of the depth-2 / depth-3 kernels (nsol_amd/csrc/nsol_pdk_plan.hpp) on a CPU:
// no HIP, no library, this file and that header alone.
//
//   pdk_plan_check            the candidate lists and plan lists of a fixed set of shapes
//                             and knobs as JSON (tests/pdk_plan_lists.json is this output)
//   pdk_plan_check --constants  kRounds kFinalRounds kFinalBand
//   pdk_plan_check --replay   drives the sampling state machine from standard input, one
//                             command per line, and prints one line per answer:
//     plan NAME N             a new exploring plan of N candidates
//     launch NAME S           a launch (S = 1: it may be a sample)  -> run C timed|untimed|settled
//     sample NAME C MS        the timed launch of candidate C took MS milliseconds
//     lost NAME C             ... or its time could not be read
//     poll NAME               settle if every owed sample is in     -> chosen C
//     owed NAME               samples still to issue                -> owed N
//     donation S U [FRESH]    launches plan S's long runs give up for plan U; U = "-":
//                             not made yet, it would list FRESH candidates -> donation N
// (tests/test_pdk_plan_host.py)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../../nsol_amd/csrc/nsol_pdk_plan.hpp"

using namespace nsol_pdk;

static const int kCus = 256;    // what the library assumes where it cannot ask a device

static void print_config(const Config &c, const char *sep) {
  printf("%s{\"nw\": %d, \"pf2\": %d, \"trimmed\": %d, \"lxb\": %d, \"rows\": %d, \"xv\": %d, "
         "\"ntx\": %d, \"nty\": %d, \"split\": %d, \"zchunk\": %lld, \"cost\": %.17g}",
         sep, c.nw, c.pf2, c.trimmed, c.q.lxb, c.q.rows, c.q.xv, c.q.ntx, c.q.nty, c.q.split,
         (long long)c.zchunk, c.cost);
}

static bool g_first_case = true;

// One case: the candidates of `key` under the knobs `t` and the list its new plan gets
// (has_shifted, settled3: nsol_pdk::list_kind).  A knob that pins the geometry: no plan,
// the launch takes the first candidate.
static void print_case(const char *name, const Tuning &t, PlanKey key, bool has_shifted = false,
                       const Config *settled3 = nullptr) {
  std::vector<Config> cand, list;
  const char *kind_name = "forced";
  if (geometry_forced(t)) {
    cand = candidates(t, key, kCus);
    if (!cand.empty()) list.push_back(cand[0]);
  } else {
    cand = plan_candidates(t, key, kCus);
    if (!cand.empty()) {
      static const char *names[] = {"single", "seeded", "short", "shifted", "full"};
      const ListKind kind = list_kind(t, key, cand, settled3, has_shifted);
      kind_name = names[kind];
      list = plan_list(cand, kind, key.nz, settled3);
    }
  }
  if (cand.empty()) kind_name = "none";
  printf("%s\n {\"case\": \"%s\", \"kind\": \"%s\", \"candidates\": %d,\n  \"head\": [",
         g_first_case ? "" : ",", name, kind_name, (int)cand.size());
  g_first_case = false;
  for (int i = 0; i < (int)cand.size() && i < 20; ++i) print_config(cand[i], i ? ",\n    " : "\n    ");
  printf("],\n  \"list\": [");
  for (int i = 0; i < (int)list.size(); ++i) print_config(list[i], i ? ",\n    " : "\n    ");
  printf("]}");
}

static PlanKey key_of(int esize, int k, int64_t nz, int64_t ny, int64_t nx, int form,
                      int64_t pitch = 0) {
  return PlanKey{0, esize, k, nz, ny, nx, pitch, form};
}

static int print_lists() {
  const Tuning def;
  printf("[");
  // 1: 512^3
  print_case("512^3 K=3 unshifted, full", def, key_of(4, 3, 512, 512, 512, 0));
  print_case("512^3 K=3 shifted", def, key_of(4, 3, 512, 512, 512, 1));
  print_case("512^3 K=3 unshifted, a shifted plan exists: short", def,
             key_of(4, 3, 512, 512, 512, 0), true);
  {
    // the depth-3 plan has settled on the model's best shifted tiling
    const std::vector<Config> c3 = plan_candidates(def, key_of(4, 3, 512, 512, 512, 1), kCus);
    print_case("512^3 K=2 seeded by a settled depth-3 plan", def, key_of(4, 2, 512, 512, 512, 0),
               true, &c3[0]);
  }
  print_case("512^3 K=2 unseeded", def, key_of(4, 2, 512, 512, 512, 0));
  // 2: 256^3
  print_case("256^3 K=3 unshifted", def, key_of(4, 3, 256, 256, 256, 0));
  print_case("256^3 K=3 shifted", def, key_of(4, 3, 256, 256, 256, 1));
  // 3: rows that are not whole vectors (12 waves only), and an odd plane count
  print_case("nz=512 ny=512 nx=511 K=3 unshifted", def, key_of(4, 3, 512, 512, 511, 0));
  print_case("nz=511 ny=512 nx=512 K=3 unshifted", def, key_of(4, 3, 511, 512, 512, 0));
  // 4: float64
  print_case("nz=300 ny=200 nx=1000 float64 K=3 unshifted", def, key_of(8, 3, 300, 200, 1000, 0));
  print_case("nz=300 ny=200 nx=1000 float64 K=3 shifted", def, key_of(8, 3, 300, 200, 1000, 1));
  // 5: rows at a pitch
  print_case("nz=256 ny=256 nx=510 pitch=512 K=3", def, key_of(4, 3, 256, 256, 510, 0, 512));
  // 6: below tune_min_mvox
  print_case("128^3 K=3 unshifted", def, key_of(4, 3, 128, 128, 128, 0));
  print_case("128^3 K=3 shifted", def, key_of(4, 3, 128, 128, 128, 1));
  // 7: 512^3 under knobs
  struct Knob { const char *name; int Tuning::*field; int value; };
  const Knob knobs[] = {{"pf2=0", &Tuning::pf2, 0},         {"split=0", &Tuning::split, 0},
                        {"xcd_map=0", &Tuning::xcd_map, 0}, {"xcd_map=2", &Tuning::xcd_map, 2},
                        {"zchunk=64", &Tuning::zchunk, 64}};
  for (int form = 0; form < 2; ++form) {
    Tuning t;
    t.nw = 12; t.ntx = 4; t.rows = 21;
    std::string name = std::string("512^3 K=3 ") + (form ? "shifted" : "unshifted");
    print_case((name + " nw=12 ntx=4 rows=21").c_str(), t, key_of(4, 3, 512, 512, 512, form));
    for (const Knob &kn : knobs) {
      Tuning u;
      u.*kn.field = kn.value;
      print_case((name + " " + kn.name).c_str(), u, key_of(4, 3, 512, 512, 512, form));
    }
  }
  // 8: nothing fits
  print_case("nz=8 ny=8192 nx=8192: a plane of 2^30 / 4 bytes", def,
             key_of(4, 3, 8, 8192, 8192, 0));
  print_case("nz=64 ny=4096 nx=4100: fewer than 16 planes in 2^30 bytes", def,
             key_of(4, 3, 64, 4096, 4100, 0));
  print_case("nz=64 ny=4096 nx=4096: 16 planes in 2^30 bytes, z-chunks of 8 still fit", def,
             key_of(4, 3, 64, 4096, 4096, 0));
  {
    Tuning t;
    t.rows = 200;     // (768 lanes in rows of at least 4)
    print_case("512^3 K=3 rows=200: more rows than fit", t, key_of(4, 3, 512, 512, 512, 0));
  }
  printf("\n]\n");
  return 0;
}

static int replay() {
  setvbuf(stdout, nullptr, _IOLBF, 0);      // the test reads each answer before it goes on
  std::map<std::string, Plan> plans;
  char line[256], cmd[32], a[64], b[64];
  while (fgets(line, sizeof line, stdin)) {
    double x = 0.0, y = 0.0;
    a[0] = b[0] = 0;
    const int n = sscanf(line, "%31s %63s %63s %lf", cmd, a, b, &y);
    if (n < 2) continue;
    if (n >= 3) x = atof(b);
    if (!strcmp(cmd, "plan")) {
      plans[a] = plan_make(std::vector<Config>((size_t)x), false);
      continue;
    }
    if (!strcmp(cmd, "donation")) {
      if (!plans.count(a) || (strcmp(b, "-") && !plans.count(b))) return 2;
      const Plan fresh = plan_make(std::vector<Config>((size_t)y), y < 2);
      printf("donation %d\n", plan_donation(plans[a], strcmp(b, "-") ? plans[b] : fresh));
      continue;
    }
    if (!plans.count(a)) return 2;
    Plan &P = plans[a];
    const int c = (int)x;
    if (!strcmp(cmd, "launch")) {
      plan_settle(P);
      if (P.chosen >= 0) {
        printf("run %d settled\n", P.chosen);
      } else {
        const PlanNext nx = plan_next(P, c != 0);
        if (nx.timed) P.issued[nx.cand]++;
        printf("run %d %s\n", nx.cand, nx.timed ? "timed" : "untimed");
      }
    } else if (!strcmp(cmd, "sample") || !strcmp(cmd, "lost")) {
      if (c < 0 || c >= (int)P.cand.size()) return 2;
      if (cmd[0] == 's') plan_record(P, c, (float)y);
      else plan_lost(P, c);
    } else if (!strcmp(cmd, "poll")) {
      plan_settle(P);
      printf("chosen %d\n", P.chosen);
    } else if (!strcmp(cmd, "owed")) {
      printf("owed %d\n", plan_owed(P));
    } else {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--replay")) return replay();
  if (argc > 1 && !strcmp(argv[1], "--constants"))
    return printf("%d %d %.9g\n", kRounds, kFinalRounds, (double)kFinalBand) < 0;
  return print_lists();
}
