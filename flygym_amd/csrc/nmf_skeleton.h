// nmf_skeleton.h — the model on the host: the NMFMODEL blob parser, and the match of the model's skeleton against the kernel
// families of nmf_families.h with the tree tables the chosen family sweeps.  Part of nmf_capi.hip's translation unit.
//
// Plain C++ without HIP; a failure is a text for the caller to report.  scripts/micro/classify_check.cpp runs it on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "nmf_families.h"

struct HostArray {
  std::vector<float> f;
  std::vector<int32_t> i;
  bool is_int = false;
  int64_t count = 0;
};

struct nmf_model {
  std::vector<uint8_t> blob;
  std::vector<std::pair<std::string, HostArray>> arrays;
  int nq = 0, nv = 0, nu = 0, nb = 0, nseg = 0, ng = 0, nsite = 0, nsensor = 0, max_iter = 100;
  int star[4] = {0, 0, 0, 0};
  const HostArray* find(const char* name) const {
    for (auto& kv : arrays) if (kv.first == name) return &kv.second;
    return nullptr;
  }
};

namespace {

struct BlobEntry {
  char name[32];
  uint32_t dtype, ndim;
  int64_t shape[4];
  int64_t offset, nbytes;
};

// The model of an NMFMODEL v4 blob; null with the reason in `err`
nmf_model* parse_model(const void* blob, size_t nbytes, std::string& err) {
  if (!blob || nbytes < 16 || memcmp(blob, "NMFMODEL", 8) != 0) { err = "nmf_model_create: not an NMFMODEL blob"; return nullptr; }
  auto* m = new nmf_model();
  m->blob.assign((const uint8_t*)blob, (const uint8_t*)blob + nbytes);
  uint32_t version, n;
  memcpy(&version, m->blob.data() + 8, 4);
  memcpy(&n, m->blob.data() + 12, 4);
  if (version != 4) { delete m; err = "nmf_model_create: unsupported blob version (this library reads NMFMODEL v4)"; return nullptr; }
  if ((uint64_t)n > (nbytes - 16) / sizeof(BlobEntry)) { delete m; err = "nmf_model_create: entry table does not fit the blob"; return nullptr; }
  const BlobEntry* e = (const BlobEntry*)(m->blob.data() + 16);
  for (uint32_t k = 0; k < n; ++k) {
    HostArray a;
    int64_t c = 1;
    bool bad = e[k].ndim > 4 || e[k].dtype > 1 || e[k].offset < 0 || e[k].nbytes < 0;
    for (uint32_t d = 0; !bad && d < e[k].ndim; ++d) {
      bad = e[k].shape[d] < 0 || (e[k].shape[d] > 0 && c > (int64_t)nbytes / e[k].shape[d]);
      c *= e[k].shape[d];
    }
    a.count = c;
    const int64_t elem = e[k].dtype == 0 ? 8 : 4;
    if (bad || (uint64_t)e[k].offset > nbytes || (uint64_t)e[k].nbytes > nbytes - (uint64_t)e[k].offset || c * elem > e[k].nbytes) {
      delete m; err = "nmf_model_create: truncated or malformed blob entry"; return nullptr;
    }
    if (e[k].dtype == 0) {
      const double* src = (const double*)(m->blob.data() + e[k].offset);
      a.f.resize((size_t)c);
      for (int64_t i = 0; i < c; ++i) a.f[(size_t)i] = (float)src[i];
    } else {
      a.is_int = true;
      a.i.resize((size_t)c);
      if (c) memcpy(a.i.data(), m->blob.data() + e[k].offset, sizeof(int32_t) * (size_t)c);      // (an empty vector has no data())
    }
    char nm[33];
    memcpy(nm, e[k].name, 32); nm[32] = 0;
    m->arrays.emplace_back(std::string(nm), std::move(a));
  }
  auto need = [&](const char* nm) -> const HostArray* {
    const HostArray* a = m->find(nm);
    if (!a) err = std::string("nmf_model_create: blob lacks entry ") + nm;
    return a;
  };
  const HostArray *bp = need("body_parent"), *db = need("dof_body"), *at = need("act_type"), *sb = need("seg_body"),
                  *gb = need("geom_body"), *si = need("site_body"), *ns = need("n_sensor"), *os = need("opt_solver"),
                  *star = need("star");
  if (!bp || !db || !at || !sb || !gb || !si || !ns || !os || !star) { delete m; return nullptr; }
  m->nb = (int)bp->count; m->nv = (int)db->count; m->nq = m->nv + 1; m->nu = (int)at->count;
  m->nseg = (int)sb->count; m->ng = (int)gb->count; m->nsite = (int)si->count;
  m->nsensor = ns->i[0]; m->max_iter = os->i[0];
  for (int k = 0; k < 4; ++k) m->star[k] = star->i[(size_t)k];
  return m;
}

// The skeleton's kernel family and, for the families with tree sweeps, the tree tables in breadth-first order
struct Skeleton {
  int topo = -1;
  std::vector<int> tree_body, child_start, child_count, lvl_start;    // lvl_start: starts of levels 0..maxd and the end
};

// Whether the model is the skeleton a star family's kernels hard-wire (the per-leg hinge layout, the control cap)
bool is_skeleton_of(const nmf::Family& f, const nmf_model* model) {
  const HostArray* bp = model->find("body_parent");
  const HostArray* dn = model->find("body_dofnum");
  if (!dn || model->nu > f.ctrl) return false;
  if (f.legs_only()) {      // the compiler found a star of chains (model->star: is one, legs, dofs and bodies per leg)
    bool ok = model->star[0] == 1 && model->star[1] == f.nleg && model->star[2] == f.ndl && model->star[3] == f.nbl &&
              dn->is_int && (int)dn->i.size() == f.nb && dn->i[0] == 6;
    for (int b = 1; ok && b < f.nb; ++b) ok = dn->i[(size_t)b] == f.dofs[(b - 1) % f.nbl];
    return ok;
  }
  // the full-body skeletons (ALL_BIOLOGICAL, ALL_POSSIBLE): identical leg chains at the END of the body order, the rest of
  // the body between the root and the legs -> hybrid kernels (legs unrolled, rest as a tree)
  const int nb = model->nb;
  bool ok = bp && nb == f.nb && model->nv == f.nv && (int)dn->i.size() == nb && dn->i[0] == 6;
  int rest_v = 0;
  for (int bb = 1; ok && bb < f.lb0; ++bb) { rest_v += dn->i[(size_t)bb]; ok = bp->i[(size_t)bb] >= 0 && bp->i[(size_t)bb] < f.lb0 && bp->i[(size_t)bb] < bb; }
  ok = ok && rest_v == f.rest_v;
  for (int bb = f.lb0; ok && bb < nb; ++bb) {
    const int l = (bb - f.lb0) % f.nbl;
    ok = dn->i[(size_t)bb] == f.dofs[l] && bp->i[(size_t)bb] == (l == 0 ? 0 : bb - 1);
  }
  return ok;
}

// Fills `sk`; returns null, or the reason no kernel takes the model
const char* classify_skeleton(const nmf_model* model, Skeleton& sk) {
  // a star family whose skeleton this is; anything else (custom skeletons): the smaller general-tree family that holds the
  // model's dofs and actuators, else the larger one
  const nmf::Family *fam = nullptr, *fit = nullptr, *big = nullptr;
  for (const nmf::Family& f : nmf::kFamilies) {
    if (f.star) { if (!fam && is_skeleton_of(f, model)) fam = &f; continue; }
    big = &f;
    if (!fit && model->nv <= f.nv && model->nu <= f.ctrl) fit = &f;
  }
  if (!fam) fam = fit ? fit : big;
  sk.topo = fam->id;
  std::vector<int> &tree_body = sk.tree_body, &child_start = sk.child_start, &child_count = sk.child_count, &lvl_start = sk.lvl_start;
  if (fam->tree_tables()) {
    const HostArray* bp = model->find("body_parent");
    const HostArray* dn = model->find("body_dofnum");
    const HostArray* gb = model->find("geom_body");
    if (!bp || !dn || !gb || model->nb > big->nb || model->nv > big->nv || dn->i.empty() || dn->i[0] != 6)
      return "nmf_batch_create: the general-tree kernel takes a free-floating root and up to 72 bodies / 216 dofs";
    const int nb = model->nb;
    // bodies the tree tables cover (hybrid: root + rest; tree kernels: all)
    std::vector<char> in_tree((size_t)nb, 1);
    if (fam->hybrid()) std::fill(in_tree.begin() + fam->lb0, in_tree.end(), 0);
    for (int bb = 1; bb < nb; ++bb)
      if (bp->i[(size_t)bb] < 0 || bp->i[(size_t)bb] >= bb) return "nmf_batch_create: bodies must be ordered parents first";
    for (size_t g = 1; g < gb->i.size(); ++g)
      if (gb->i[g] < gb->i[g - 1]) return "nmf_batch_create: contact geoms must be ordered by body";
    // breadth-first order: level by level, the children of a body contiguous
    std::vector<int> depth((size_t)nb, 0);
    int maxd = 0;
    for (int bb = 1; bb < nb; ++bb) {
      depth[(size_t)bb] = depth[(size_t)bp->i[(size_t)bb]] + 1;
      if (in_tree[(size_t)bb]) maxd = std::max(maxd, depth[(size_t)bb]);
    }
    if (maxd + 2 > 18) return "nmf_batch_create: kinematic tree deeper than 16 levels";
    tree_body.push_back(0); lvl_start.push_back(0);
    child_start.assign((size_t)nb, 0); child_count.assign((size_t)nb, 0);
    for (int lv = 0; lv <= maxd; ++lv) {
      const int k0 = lvl_start[(size_t)lv], k1 = (int)tree_body.size();
      lvl_start.push_back(k1);
      for (int k = k0; k < k1; ++k) {
        const int par = tree_body[(size_t)k];
        child_start[(size_t)par] = (int)tree_body.size();
        for (int bb = 1; bb < nb; ++bb) if (bp->i[(size_t)bb] == par && in_tree[(size_t)bb]) { tree_body.push_back(bb); child_count[(size_t)par]++; }
      }
      if (k1 - k0 > nmf::kWave) return "nmf_batch_create: more than 64 bodies on one tree level";
    }
    // lvl_start has maxd + 2 entries: starts of levels 0..maxd and the end
  }
  if (model->ng > 2 * nmf::kWave) return "nmf_batch_create: more than 128 contact geoms";
  if (model->nu > fam->ctrl) return "nmf_batch_create: too many actuators (48 for the leg skeletons, 224 otherwise)";
  return nullptr;
}

// Hybrid families, fast level passes: DevModel::rest_pack of the skeleton's rest of the body, false where its shape needs the
// table-driven passes (a body without exactly three dofs, more than kRestLevels levels or 8 bodies on one)
bool rest_pack_words(const nmf_model* model, const Skeleton& sk, std::vector<int>& pack) {
  const HostArray *bp = model->find("body_parent"), *dn = model->find("body_dofnum"), *da = model->find("body_dofadr");
  const std::vector<int> &tree_body = sk.tree_body, &child_start = sk.child_start, &child_count = sk.child_count, &lvl_start = sk.lvl_start;
  const int nl = (int)lvl_start.size() - 2;                 // levels below the root
  bool fast = da && nl <= nmf::kRestLevels;
  pack.assign((size_t)nmf::kRestLevels * 16, -1);
  for (int lv = 1; fast && lv <= nl; ++lv) {
    const int k0 = lvl_start[(size_t)lv], k1 = lvl_start[(size_t)lv + 1];
    fast = k1 - k0 <= 8;
    for (int k = k0; fast && k < k1; ++k) {
      const int bb = tree_body[(size_t)k];
      fast = dn->i[(size_t)bb] == 3 && da->i[(size_t)bb] < 256 && child_count[(size_t)bb] < 256 && child_start[(size_t)bb] < 256;
      pack[(size_t)((lv - 1) * 8 + (k - k0)) * 2] = bb | (bp->i[(size_t)bb] << 8) | (da->i[(size_t)bb] << 16) | (child_count[(size_t)bb] << 24);
      pack[(size_t)((lv - 1) * 8 + (k - k0)) * 2 + 1] = child_start[(size_t)bb] | (k << 8);
    }
  }
  return fast;
}

}  // namespace
