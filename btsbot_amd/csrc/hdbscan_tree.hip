// btsbot_hdbscan_tree, btsbot_hdbscan_model: the HDBSCAN hierarchy, condensed tree, stabilities and selection from a
// spanning tree of the mutual-reachability graph.  Host only: no stream, no GPU call, nothing of common.h (DESIGN.md
// section 4v; tests/hdbscan_ref.py is the float64 restatement, tests/test_hdbscan_host.py compares the two exactly).
//
//   1 sort the edges by weight
//   2 the TIE-INVARIANT dendrogram: all edges of one weight are applied at once, every set of old components they join
//     becomes one node with two or more children.  The finds of a weight are taken before its unions, so a node's
//     children are the components as they stood below that weight -- whatever order the edges came in and whichever of
//     several minimum spanning trees they are.
//   3 the condensed tree, top-down (a child is real when its size >= min_cluster_size), lambda = 1 / w
//   4 canonical numbering: clusters by (smallest row, size descending), entries by (parent, child)
//   5 stabilities in that order, the selection bottom-up, labels and probabilities
// O(n log n): two sorts, a union-find, and passes over O(n) nodes.
// btsbot_hdbscan_model is the same pass (one function, tree_pass) handing out the tables a prediction walks -- per row
// the cluster it fell out of and its lambda, per cluster parent, birth, label, the strength's denominator and the largest
// lambda of its subtree -- and the GLOSH score of the fitted rows (tests/hdbscan_predict_ref.py).
#include <stdarg.h>
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/btsbot_hip.h"

void btsbot_set_error(const char* fmt, ...);

namespace {

struct Dsu {
  std::vector<int32_t> p;
  explicit Dsu(int64_t n) : p((size_t)n) { std::iota(p.begin(), p.end(), 0); }
  int32_t find(int32_t x) {
    while (p[x] != x) {
      p[x] = p[p[x]];
      x = p[x];
    }
    return x;
  }
};

struct Cluster {
  int32_t minrow, size, parent;   // parent: a cluster, in discovery numbering; -1 for the root
  double birth;
};

struct Entry {
  int64_t parent, child;   // cluster ids >= n once renumbered; child < n is a row
  double lam;
  int64_t size;
};

// what btsbot_hdbscan_model hands out of the pass: per row the cluster it fell out of and the lambda, per cluster (in
// the canonical numbering less n) its parent, birth, the label and largest lambda of its nearest selected
// ancestor-or-self, and the largest lambda of its subtree
struct Tables {
  std::vector<int32_t> fell, parent, label;
  std::vector<double> lam_row, birth, max_lambda, death;
  double lam_zero = 1.0;
};

// the whole pass; `out` (or nullptr) receives the tables
int tree_pass(const char* who, const int64_t* edges, const float* weights, int64_t n_edges, int64_t n,
              int min_cluster_size, int method, int allow_single_cluster, int64_t* labels, double* prob,
              int64_t* cond_parent, int64_t* cond_child, double* cond_lambda, int64_t* cond_size,
              int64_t cond_capacity, int64_t* n_cond, Tables* out) {
  if (n < 0 || n > 0x7fffffffLL / 2 || n_edges < 0 || n_edges >= std::max<int64_t>(n, 1) || min_cluster_size < 2 ||
      (method != BTSBOT_HDBSCAN_EOM && method != BTSBOT_HDBSCAN_LEAF)) {
    btsbot_set_error("%s: need 0 <= n < 2^30, 0 <= n_edges < n, min_cluster_size >= 2 and a known method (n=%lld "
                     "n_edges=%lld min_cluster_size=%d method=%d)", who, (long long)n, (long long)n_edges,
                     min_cluster_size, method);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((n > 0 && (labels == nullptr || prob == nullptr)) || n_cond == nullptr ||
      (n_edges > 0 && (edges == nullptr || weights == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  for (int64_t i = 0; i < n; ++i) {
    labels[i] = -1;
    prob[i] = 0.0;
  }
  *n_cond = 0;
  if (out != nullptr) {
    out->fell.assign((size_t)n, -1);
    out->lam_row.assign((size_t)n, 0.0);
  }
  if (n_edges == 0) return BTSBOT_OK;
  for (int64_t e = 0; e < n_edges; ++e) {
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= n || b < 0 || b >= n || a == b || !(weights[e] >= 0.0f)) {
      btsbot_set_error("%s: edge %lld = (%lld, %lld) of weight %g: rows must be distinct and in [0, n), weights >= 0",
                       who, (long long)e, (long long)a, (long long)b, (double)weights[e]);
      return BTSBOT_ERR_INVALID_ARG;
    }
  }

  // ---- 1, 2: the dendrogram.  Nodes 0..n-1 are the rows, n.. the merges.
  std::vector<int32_t> order((size_t)n_edges);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return weights[x] < weights[y]; });
  Dsu dsu(n);
  std::vector<int32_t> node_of((size_t)n);      // at a union-find root: the node of its component
  std::iota(node_of.begin(), node_of.end(), 0);
  std::vector<float> node_w;                     // of the merges, by node - n
  std::vector<int32_t> node_size((size_t)n, 1), node_min((size_t)n);
  std::iota(node_min.begin(), node_min.end(), 0);
  std::vector<std::pair<int32_t, int32_t>> link;    // (parent node, child node), in no particular order
  std::vector<int32_t> fresh((size_t)n, -1), seen((size_t)n, -1);   // by union-find root, stamped with the weight group
  std::vector<int32_t> fresh_node((size_t)n, 0);
  std::vector<std::pair<int32_t, int32_t>> olds, pairs;
  link.reserve((size_t)(2 * n_edges));
  int32_t group = 0;
  for (int64_t at = 0; at < n_edges; ++group) {
    int64_t end = at;
    while (end < n_edges && weights[order[end]] == weights[order[at]]) ++end;
    olds.clear();
    pairs.clear();
    for (int64_t i = at; i < end; ++i) {
      const int32_t ra = dsu.find((int32_t)edges[2 * order[i]]), rb = dsu.find((int32_t)edges[2 * order[i] + 1]);
      for (int32_t r : {ra, rb})
        if (seen[r] != group) {
          seen[r] = group;
          olds.emplace_back(r, node_of[r]);
        }
      pairs.emplace_back(ra, rb);
    }
    for (auto& pr : pairs) {
      const int32_t ra = dsu.find(pr.first), rb = dsu.find(pr.second);
      if (ra != rb) dsu.p[std::max(ra, rb)] = std::min(ra, rb);
    }
    for (auto& od : olds) {
      const int32_t r = dsu.find(od.first);
      if (fresh[r] != group) {
        fresh[r] = group;
        fresh_node[r] = (int32_t)node_size.size();
        node_w.push_back(weights[order[at]]);
        node_size.push_back(0);
        node_min.push_back((int32_t)n);
      }
      const int32_t v = fresh_node[r];
      link.emplace_back(v, od.second);
      node_size[v] += node_size[od.second];
      node_min[v] = std::min(node_min[v], node_min[od.second]);
    }
    for (auto& od : olds) {
      const int32_t r = dsu.find(od.first);
      node_of[r] = fresh_node[r];
    }
    at = end;
  }
  const int32_t n_nodes = (int32_t)node_size.size(), root = n_nodes - 1;
  if (node_size[root] != n_edges + 1) {
    btsbot_set_error("%s: the %lld edges are not a spanning tree of the rows they name (a cycle, or several trees)", who,
                     (long long)n_edges);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // children as a CSR over the merges
  std::vector<int32_t> kid_start((size_t)(n_nodes - n) + 1, 0), kid(link.size());
  for (auto& l : link) ++kid_start[l.first - n + 1];
  for (size_t i = 1; i < kid_start.size(); ++i) kid_start[i] += kid_start[i - 1];
  {
    std::vector<int32_t> fill(kid_start.begin(), kid_start.end() - 1);
    for (auto& l : link) kid[fill[l.first - n]++] = l.second;
  }
  auto kids_of = [&](int32_t v) { return std::make_pair(kid.begin() + kid_start[v - n], kid.begin() + kid_start[v - n + 1]); };

  // ---- 3: the condensed tree
  double lam_zero = 1.0;
  {
    float least = 0.0f;   // the smallest positive weight
    for (float w : node_w)
      if (w > 0.0f && (least == 0.0f || w < least)) least = w;
    if (least > 0.0f) lam_zero = 1.0 / (double)least;
  }
  auto lam_of = [&](int32_t v) { return node_w[v - n] == 0.0f ? lam_zero : 1.0 / (double)node_w[v - n]; };
  std::vector<Cluster> clusters;
  clusters.push_back({node_min[root], node_size[root], -1, 0.0});
  std::vector<Entry> entries;
  entries.reserve((size_t)n_edges + 1);
  std::vector<std::pair<int32_t, int32_t>> stack{{root, 0}};
  std::vector<int32_t> walk;
  while (!stack.empty()) {
    const auto [v, c] = stack.back();
    stack.pop_back();
    const double lam = lam_of(v);
    const auto [k0, k1] = kids_of(v);
    int real = 0;
    for (auto k = k0; k != k1; ++k) real += node_size[*k] >= min_cluster_size;
    for (auto k = k0; k != k1; ++k) {
      const int32_t x = *k;
      if (node_size[x] >= min_cluster_size) {
        if (real == 1) {
          stack.emplace_back(x, c);
        } else {
          clusters.push_back({node_min[x], node_size[x], c, lam});
          const int32_t id = (int32_t)clusters.size() - 1;
          entries.push_back({c, -(int64_t)id - 1, lam, node_size[x]});   // a cluster as -(id + 1) until renumbered
          stack.emplace_back(x, id);
        }
        continue;
      }
      walk.assign(1, x);   // every row under x falls out of c here
      while (!walk.empty()) {
        const int32_t y = walk.back();
        walk.pop_back();
        if (y < n) {
          entries.push_back({c, y, lam, 1});
        } else {
          const auto [y0, y1] = kids_of(y);
          walk.insert(walk.end(), y0, y1);
        }
      }
    }
  }

  // ---- 4: canonical numbering
  const int32_t nc = (int32_t)clusters.size();
  std::vector<int32_t> by_rank((size_t)nc), new_id((size_t)nc);
  std::iota(by_rank.begin(), by_rank.end(), 0);
  std::sort(by_rank.begin(), by_rank.end(), [&](int32_t x, int32_t y) {
    return clusters[x].minrow != clusters[y].minrow ? clusters[x].minrow < clusters[y].minrow
                                                    : clusters[x].size > clusters[y].size;
  });
  for (int32_t i = 0; i < nc; ++i) new_id[by_rank[i]] = i;
  std::vector<double> birth((size_t)nc);
  std::vector<int32_t> par((size_t)nc);
  for (int32_t k = 0; k < nc; ++k) {
    birth[new_id[k]] = clusters[k].birth;
    par[new_id[k]] = clusters[k].parent < 0 ? -1 : new_id[clusters[k].parent];
  }
  for (auto& e : entries) {
    e.parent = n + new_id[e.parent];
    if (e.child < 0) e.child = n + new_id[-e.child - 1];
  }
  std::sort(entries.begin(), entries.end(), [](const Entry& x, const Entry& y) {
    return x.parent != y.parent ? x.parent < y.parent : x.child < y.child;
  });
  *n_cond = (int64_t)entries.size();
  if (cond_parent != nullptr || cond_child != nullptr || cond_lambda != nullptr || cond_size != nullptr) {
    if (cond_parent == nullptr || cond_child == nullptr || cond_lambda == nullptr || cond_size == nullptr ||
        cond_capacity < (int64_t)entries.size()) {
      btsbot_set_error("%s: the condensed tree holds %lld entries; all four arrays or none, of that capacity (got %lld)",
                       who, (long long)entries.size(), (long long)cond_capacity);
      return BTSBOT_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < entries.size(); ++i) {
      cond_parent[i] = entries[i].parent;
      cond_child[i] = entries[i].child;
      cond_lambda[i] = entries[i].lam;
      cond_size[i] = entries[i].size;
    }
  }

  // ---- 5: stabilities, selection, labels, probabilities
  std::vector<double> row_sum((size_t)nc, 0.0), child_sum((size_t)nc, 0.0), max_lam((size_t)nc, 0.0), best((size_t)nc, 0.0);
  std::vector<int32_t> fell((size_t)n, -1), first_kid((size_t)nc + 1, 0);
  std::vector<double> lam_row((size_t)n, 0.0);
  std::vector<int32_t> kid_list;   // child clusters, grouped by parent in ascending order: the entries are sorted so
  for (const Entry& e : entries) {
    const int32_t c = (int32_t)(e.parent - n);
    max_lam[c] = std::max(max_lam[c], e.lam);
    if (e.child < n) {
      row_sum[c] = row_sum[c] + (e.lam - birth[c]);
      fell[e.child] = c;
      lam_row[e.child] = e.lam;
    } else {
      child_sum[c] = child_sum[c] + (double)e.size * (e.lam - birth[c]);
      kid_list.push_back((int32_t)(e.child - n));
      ++first_kid[c + 1];
    }
  }
  for (int32_t c = 0; c < nc; ++c) first_kid[c + 1] += first_kid[c];
  std::vector<uint8_t> flag((size_t)nc, 0);
  for (int32_t c = nc - 1; c >= 0; --c) {
    const bool leaf = first_kid[c] == first_kid[c + 1];
    if (method == BTSBOT_HDBSCAN_LEAF) {
      flag[c] = leaf;
      continue;
    }
    const double stab = row_sum[c] + child_sum[c];
    if (leaf) {
      flag[c] = 1;
      best[c] = stab;
      continue;
    }
    double s = 0.0;
    for (int32_t i = first_kid[c]; i < first_kid[c + 1]; ++i) s = s + best[kid_list[i]];
    flag[c] = !(s > stab);
    best[c] = s > stab ? s : stab;
  }
  if (!allow_single_cluster) flag[0] = 0;
  std::vector<int32_t> sel((size_t)nc, -1), number((size_t)nc, -1);   // the nearest selected ancestor-or-self
  int32_t count = 0;
  for (int32_t c = 0; c < nc; ++c) {
    const int32_t up = par[c] >= 0 ? sel[par[c]] : -1;
    sel[c] = up >= 0 ? up : (flag[c] ? c : -1);
    if (sel[c] == c) number[c] = count++;   // ascending id = ascending smallest row among disjoint clusters
  }
  for (int64_t r = 0; r < n; ++r) {
    if (fell[r] < 0 || sel[fell[r]] < 0) continue;
    const int32_t s = sel[fell[r]];
    labels[r] = number[s];
    prob[r] = max_lam[s] == 0.0 ? 1.0 : std::min(lam_row[r], max_lam[s]) / max_lam[s];
  }
  if (out != nullptr) {
    out->lam_zero = lam_zero;
    out->label.assign((size_t)nc, -1);
    out->max_lambda.assign((size_t)nc, 0.0);
    out->death = max_lam;
    for (int32_t c = 0; c < nc; ++c)
      if (sel[c] >= 0) {
        out->label[c] = number[sel[c]];
        out->max_lambda[c] = max_lam[sel[c]];
      }
    for (int32_t c = nc - 1; c > 0; --c)   // (a parent stands before its children)
      out->death[par[c]] = std::max(out->death[par[c]], out->death[c]);
    out->fell = std::move(fell);
    out->lam_row = std::move(lam_row);
    out->parent = std::move(par);
    out->birth = std::move(birth);
  }
  return BTSBOT_OK;
}

}  // namespace

extern "C" int btsbot_hdbscan_tree(const int64_t* edges, const float* weights, int64_t n_edges, int64_t n,
                                   int min_cluster_size, int method, int allow_single_cluster, int64_t* labels,
                                   double* prob, int64_t* cond_parent, int64_t* cond_child, double* cond_lambda,
                                   int64_t* cond_size, int64_t cond_capacity, int64_t* n_cond) {
  return tree_pass("btsbot_hdbscan_tree", edges, weights, n_edges, n, min_cluster_size, method, allow_single_cluster,
                   labels, prob, cond_parent, cond_child, cond_lambda, cond_size, cond_capacity, n_cond, nullptr);
}

extern "C" int btsbot_hdbscan_model(const int64_t* edges, const float* weights, int64_t n_edges, int64_t n,
                                    int min_cluster_size, int method, int allow_single_cluster, int32_t* row_cluster,
                                    double* row_lambda, double* outlier, int32_t* parent, double* birth, int32_t* label,
                                    double* max_lambda, double* death, int64_t cluster_capacity, int64_t* n_clusters,
                                    double* lam_zero) {
  const char* who = "btsbot_hdbscan_model";
  if (n_clusters == nullptr || lam_zero == nullptr || cluster_capacity < 0 ||
      (n > 0 && (row_cluster == nullptr || row_lambda == nullptr || outlier == nullptr))) {
    btsbot_set_error("%s: NULL argument, or a negative cluster_capacity", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  *n_clusters = 0;
  *lam_zero = 1.0;
  if (n < 0 || n > 0x7fffffffLL / 2) {   // (before anything of size n is allocated; the pass checks the rest)
    btsbot_set_error("%s: need 0 <= n < 2^30 (n=%lld)", who, (long long)n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  std::vector<int64_t> labels((size_t)n);
  std::vector<double> prob(labels.size());
  int64_t n_cond = 0;
  Tables t;
  const int rc = tree_pass(who, edges, weights, n_edges, n, min_cluster_size, method, allow_single_cluster, labels.data(),
                           prob.data(), nullptr, nullptr, nullptr, nullptr, 0, &n_cond, &t);
  if (rc != BTSBOT_OK) return rc;
  const int64_t nc = (int64_t)t.parent.size();
  if (nc > cluster_capacity || (nc > 0 && (parent == nullptr || birth == nullptr || label == nullptr ||
                                           max_lambda == nullptr || death == nullptr))) {
    btsbot_set_error("%s: the tree holds %lld clusters; the five cluster arrays need that capacity (got %lld; at most "
                     "max(n - 1, 1) are ever needed)", who, (long long)nc, (long long)cluster_capacity);
    return BTSBOT_ERR_INVALID_ARG;
  }
  for (int64_t c = 0; c < nc; ++c) {
    parent[c] = t.parent[c];
    birth[c] = t.birth[c];
    label[c] = t.label[c];
    max_lambda[c] = t.max_lambda[c];
    death[c] = t.death[c];
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t r = 0; r < n; ++r) {
    const int32_t c = t.fell[r];
    row_cluster[r] = c;
    row_lambda[r] = t.lam_row[r];
    outlier[r] = c < 0 ? nan : (t.death[c] == 0.0 ? 0.0 : 1.0 - t.lam_row[r] / t.death[c]);
  }
  *n_clusters = nc;
  *lam_zero = t.lam_zero;
  return BTSBOT_OK;
}
