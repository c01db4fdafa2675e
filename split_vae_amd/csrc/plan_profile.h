// Per-scope hipEvent timing of the step plan (bench.py's roofline table reads the scopes by name): the Profiler the plan holds by value, the Scope bracket
// around one launch set, and the optional roctx ranges of the same names.
// ONE includer (lgvae_plan.hip): everything here is in an anonymous namespace, a second translation unit would get its own Roctx singleton.
#pragma once
#include <map>
#include <string>
#include <vector>
#include <stdio.h>
#include <dlfcn.h>
#include "common.hip.h"
#include "kernels.h"

namespace {

// SV_ROCTX=1: every plan scope ("fwd.d4", "wgrad.d4", "adam_step" ...) is also a roctx range, so a `rocprofv3 --marker-trace
// --kernel-trace` timeline names the layers directly.  libroctx64 is bound at run time (no link dependency); off by default.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (!sv_knob_roctx()) return;
    void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static const Roctx& roctx() { static const Roctx r; return r; }

struct Profiler {
  // issued: FLOPs per launch the scope's chosen algorithm really multiplies (polyphase forms: fewer than the direct count `flops`)
  struct Entry { std::string name; double flops, bytes, total_ms; int launches; double issued; };
  struct Pending { int entry; hipEvent_t a, b; };
  bool on = false;
  std::string filter;                  // brackets only around launches of this name ("" = all)
  std::vector<Entry> entries;
  std::map<std::string, int> index;
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;

  bool serial() const { return on && filter.empty(); }   // the full per-kernel table wants serial launches (no side streams)
  hipEvent_t get() {
    hipEvent_t e;
    if (!pool.empty()) { e = pool.back(); pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
  }
  int find(const char* name, double flops, double bytes) {
    auto it = index.find(name);
    if (it != index.end()) return it->second;
    const int e = (int)entries.size();
    index[name] = e;
    entries.push_back(Entry{name, flops, bytes, 0.0, 0, flops});
    return e;
  }
  void enable(bool enable) {           // sv_lgvae_profile_enable
    on = enable;
    if (!enable) return;
    for (auto& pe : pending) { pool.push_back(pe.a); pool.push_back(pe.b); }
    pending.clear();
    entries.clear();
    index.clear();
  }
  int read(int max_entries, char names[][64], double* total_ms, int32_t* launches, double* flops_per_launch, double* bytes_per_launch) {   // sv_lgvae_profile_read
    for (auto& pe : pending) {
      (void)hipEventSynchronize(pe.b);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
        entries[pe.entry].total_ms += ms;
        entries[pe.entry].launches += 1;
      }
      pool.push_back(pe.a);
      pool.push_back(pe.b);
    }
    pending.clear();
    int n = (int)entries.size();
    if (n > max_entries) n = max_entries;
    for (int i = 0; i < n; ++i) {
      if (names) snprintf(names[i], 64, "%s", entries[i].name.c_str());
      if (total_ms) total_ms[i] = entries[i].total_ms;
      if (launches) launches[i] = entries[i].launches;
      if (flops_per_launch) flops_per_launch[i] = entries[i].flops;
      if (bytes_per_launch) bytes_per_launch[i] = entries[i].bytes;
    }
    return n;
  }
  int read_issued(int max_entries, double* issued_flops_per_launch) const {   // sv_lgvae_profile_read_issued: same order as read()
    int n = (int)entries.size();
    if (n > max_entries) n = max_entries;
    for (int i = 0; i < n; ++i) issued_flops_per_launch[i] = entries[i].issued;
    return n;
  }
  void destroy() {
    for (auto& pe : pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

struct Scope {   // hipEvent bracket around one launch when profiling is on
  Profiler& p; hipStream_t st; int entry = -1, entry2 = -1; hipEvent_t a = nullptr, b = nullptr, m1 = nullptr, m2 = nullptr;
  bool on, on2 = false;
  bool marked = false;
  void issued(double fl) { if (entry >= 0) p.entries[entry].issued = fl; }      // the launch set runs a strength-reduced form: FLOPs it really multiplies
  Scope(Profiler& p_, hipStream_t st_, const std::string& name, double flops, double bytes) : Scope(p_, st_, name.c_str(), flops, bytes) {}
  Scope(Profiler& p_, hipStream_t st_, const char* name, double flops, double bytes) : p(p_), st(st_), on(p_.on) {   // (a literal or a Layer's name: no string is built unless profiling books one)
    if (roctx().push) { roctx().push(name); marked = true; }
    if (on && !p.filter.empty() && p.filter != name) on = false;
    if (!on) return;
    entry = p.find(name, flops, bytes);
    a = p.get(); b = p.get();
    (void)hipEventRecord(a, st);
  }
  // a launch with a second stage (wgrad tile kernel -> slab reduce): the callee records ev[0], ev[1] between
  // the two, and the second stage is booked under its own name
  void split(const std::string& name2, double bytes2, hipEvent_t ev[2]) {
    ev[0] = ev[1] = nullptr;
    if (!p.on) return;
    on2 = p.filter.empty() || p.filter == name2;
    if (!on && !on2) return;
    if (on2) entry2 = p.find(name2.c_str(), 0, bytes2);
    m1 = ev[0] = p.get(); m2 = ev[1] = p.get();
    if (!b) b = p.get();
  }
  ~Scope() {
    if (marked) roctx().pop();
    if (!b) return;
    (void)hipEventRecord(b, st);
    if (!m1) { p.pending.push_back(Profiler::Pending{entry, a, b}); return; }
    if (on) p.pending.push_back(Profiler::Pending{entry, a, m1}); else p.pool.push_back(m1);
    if (on2) p.pending.push_back(Profiler::Pending{entry2, m2, b});
    else { p.pool.push_back(m2); p.pool.push_back(b); }
  }
};

}  // namespace
