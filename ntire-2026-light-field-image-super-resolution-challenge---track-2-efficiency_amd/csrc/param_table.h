// The model-context core of the five C model drivers (DistgSSR, EPIT, LFT, LF_InterNet, LFSSR): the packed-parameter table keyed by the reference's
// state_dict names, and the base every context derives from, with the life-cycle steps the drivers share.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "lfsr_internal.h"

struct LfsrParamTable {
  struct Slot {
    size_t off = 0, floats = 0, numel = 0;
    size_t grad_off = 0;   // parameters: offset in the flat gradient bucket
    int O = 0, C = 0, T = 0, perm = 0, ch = 0;
    bool raw = false, param = true, loaded = false;
  };
  std::map<std::string, Slot> slots;
  size_t packed_floats = 0;
  size_t n_params = 0;     // the gradient bucket: the parameters in insertion order, which is state_dict order (the map iterates alphabetically)
  float* packed = nullptr;

  // param = false: an internal entry (a second packing of a parameter under a key of its own), not in the gradient bucket
  void add(const std::string& k, int O, int C, int T, int perm = 0, int ch = 0, bool raw = false, bool param = true) {
    Slot s;
    s.O = O; s.C = C; s.T = T; s.perm = perm; s.ch = ch; s.raw = raw; s.param = param;
    s.numel = (size_t)O * C * T;
    s.floats = raw ? s.numel : lfsr_packed_weight_floats(O, C, T);
    s.off = reserve(s.floats);
    if (param) {
      s.grad_off = n_params;
      n_params += s.numel;
    }
    slots[k] = s;
  }
  // a region of the packed buffer that is no entry (what finalize or a second packing derives from the weights)
  size_t reserve(size_t floats) {
    const size_t o = packed_floats;
    packed_floats += LfsrArena::granules(floats);
    return o;
  }
  const float* w(const std::string& k) const { return packed + slots.at(k).off; }
  size_t grad_off(const std::string& k) const { return slots.at(k).grad_off; }
  size_t num_params() const { return n_params; }
  int param_offset(const char* key, size_t* off, size_t* numel) const {
    if (!key) return LFSR_E_ARG;
    auto it = slots.find(key);
    if (it == slots.end() || !it->second.param) return LFSR_E_ARG;
    if (off) *off = it->second.grad_off;
    if (numel) *numel = it->second.numel;
    return LFSR_OK;
  }
  int set_packed(void* p, size_t bytes) {
    if (!p || bytes < packed_floats * sizeof(float) || ((uintptr_t)p & 15)) return LFSR_E_ARG;
    packed = (float*)p;
    for (auto& kv : slots) kv.second.loaded = false;
    return LFSR_OK;
  }
  // load_param's shared part: the key and the element count checked, a raw entry copied.  *pack = the entry the caller still packs from
  // `data` (and then marks loaded), nullptr when nothing is left to do.
  int load_begin(const char* key, const float* data, size_t numel, void* stream, Slot** pack) {
    *pack = nullptr;
    if (!key || !data || !packed) return LFSR_E_ARG;
    auto it = slots.find(key);
    if (it == slots.end() || numel != it->second.numel) return LFSR_E_ARG;
    Slot& s = it->second;
    if (!s.raw) {
      *pack = &s;
      return LFSR_OK;
    }
    hipError_t e = hipMemcpyAsync(packed + s.off, data, numel * sizeof(float), hipMemcpyDeviceToDevice, lfsr_stream(stream));
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    s.loaded = true;
    return LFSR_OK;
  }
  // ... and the rest packed by the operator-level pack (every Winograd-domain copy of a 3x3 64 -> 64 weight)
  int load(const char* key, const float* data, size_t numel, void* stream) {
    Slot* s = nullptr;
    LFSR_RC(load_begin(key, data, numel, stream, &s));
    if (s) {
      LFSR_RC(lfsr_pack_conv_weight(data, packed + s->off, s->O, s->C, s->T, s->perm, s->ch, stream));
      s->loaded = true;
    }
    return LFSR_OK;
  }
  bool all_loaded() const {
    for (auto& kv : slots)
      if (!kv.second.loaded) return false;
    return true;
  }
};

// What every model context holds, and the life-cycle steps the drivers share: each extern "C" entry point stays one short call into these.
struct LfsrModel {
  int A = 0, s = 0;
  LfsrParamTable P;
  bool finalized = false;   // cleared by every set_packed / load_param call, set by a finalize that succeeded

  size_t packed_bytes() const { return P.packed_floats * sizeof(float); }
  int set_packed(void* p, size_t bytes) {
    finalized = false;
    return P.set_packed(p, bytes);
  }
  int load_begin(const char* key, const float* data, size_t numel, void* stream, LfsrParamTable::Slot** pack) {
    finalized = false;
    return P.load_begin(key, data, numel, stream, pack);
  }
  int load_param(const char* key, const float* data, size_t numel, void* stream) {
    finalized = false;
    return P.load(key, data, numel, stream);
  }
  bool all_loaded() const { return P.packed && P.all_loaded(); }   // what finalize requires
  // the guard of the forward / forward_train / backward entry points: operands present, a positive geometry, a finalized model, a 16-B aligned workspace
  bool run_args_ok(const void* x, const void* y, int B, int h, int w, const void* workspace) const {
    return x && y && workspace && B > 0 && h > 0 && w > 0 && finalized && !((uintptr_t)workspace & 15);
  }
};
