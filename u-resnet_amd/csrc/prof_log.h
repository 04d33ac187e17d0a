// Optional per-launch timing with HIP events on the launch stream (bench.py --breakdown / --layers, the roofline leg): the log of
// one plan.  ProfScope (net.hip) and BProf (net_bf16.hip) write it, ursn_profile_enable / ursn_profile_read switch and drain it.
#pragma once
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ursn_common.h"

struct ProfRec { int layer, pass; const char* kernel; double flops, bytes; hipEvent_t e0, e1; long l0; int launches; };

struct ProfLog {
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;   // events are reused from one read to the next
  size_t used = 0;
  ~ProfLog() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
  hipEvent_t event() {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    return pool[used++];
  }
  void enable(bool on_) { on = on_; recs.clear(); used = 0; }
  // out == NULL: only counts, all of them; otherwise drains the log.  layer_name(index) names a record's layer.
  template <class Name>
  void read(Name layer_name, ursn_prof_rec* out, int64_t max_recs, int64_t* n_out) {
    int64_t cnt = 0;
    for (size_t i = 0; i < recs.size() && (!out || cnt < max_recs); ++i) {
      const ProfRec& r = recs[i];
      float ms = 0.f;
      if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
      if (out) {
        ursn_prof_rec& o = out[cnt];
        memset(&o, 0, sizeof(o));
        snprintf(o.kernel, sizeof(o.kernel), "%s", r.kernel);
        snprintf(o.layer, sizeof(o.layer), "%s", layer_name(r.layer));
        o.pass = r.pass; o.ms = ms; o.flops = r.flops; o.bytes = r.bytes; o.launches = r.launches;
      }
      ++cnt;
    }
    *n_out = cnt;
    if (out) { recs.clear(); used = 0; }
  }
};
