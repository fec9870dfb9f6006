// Spanning-forest carry (RELP_CARRY_NETWORK): the basis of a network LP kept as a forest of the rows (device_lp.hpp: NetTree).
//
// A basic incidence column joins two rows; a basic single-entry column (an artificial, an arc at a removed s or t) is the root
// arc of its row's tree.  With sign[x] the entry of x's parent arc (as it stands in B: negated when held complemented) at x:
//   B^-1 (i, j) = sign[child[i]]  when row j lies below the arc of slot i, else 0     (entries in {0, +-1})
//   FTRAN of an arc (u, v)        alpha = +-1 on the slots of the tree path between u and v (to the roots when they are apart)
//   row p of B^-1                 sign[child[p]] on the subtree below the leaving arc
//   B^-T y                        sums along root paths
// A pivot is five launches on the handle's stream: the pricing pass, net_ftran_kernel (entering column, tree path into alpha_in),
// the ratio test of the explicit carry with alpha preselected (kernels.hip: register-resident up to 8192 rows, across workgroups
// beyond -- the reference's rule at every size, see net_enqueue_pivot), net_update_kernel (rho_p, w = B^-T alpha, the -pi shift: one thread per row walks its root path in the OLD
// forest) and net_rehang_kernel (the path from the entering endpoint to the leaving arc reversed, one thread).  No array is m x m.
#include "kernels.hpp"
#include "price_step.hpp"
#include "solver.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <thread>

#include "rat.hpp"

namespace relp {

namespace {
double now_seconds_net() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
constexpr int NET_THREADS = 256;
constexpr int NET_WAVE = 64;
}  // namespace

// ---------------------------------------------------------------------------------------------------
// Entering column (the candidates of the pricing pass, same total order as the explicit carry's ratio-test kernels) and its tree
// path: the entering endpoint u's root path is stamped, v climbs until it meets a stamp (the common ancestor) or its root.
// alpha_in = B^-1 a_q (unsigned: the ratio test applies the complemented sign); the previous path's entries are cleared first.
// ---------------------------------------------------------------------------------------------------
template <int RULE>
__global__ void __launch_bounds__(NET_THREADS) net_ftran_kernel(DeviceLP lp, NetTree t, int n_price_blocks, int mode) {
    __shared__ double s_key[NET_THREADS / NET_WAVE];
    __shared__ unsigned long long s_rank[NET_THREADS / NET_WAVE];
    Ctl* ctl = lp.ctl;
    const int tid = threadIdx.x, m = lp.m;
    const int status = ctl->status;
    const long long iters = ctl->iters, budget = ctl->budget;
    const int forced_q = ctl->forced_q;
    if (status != ST_RUNNING) return;
    if (mode == 0 && iters >= budget) {
        if (tid == 0) ctl_budget(*ctl);
        return;
    }
    const int old_len = t.state[1];
    for (int k = tid; k < old_len; k += NET_THREADS) lp.alpha_in[t.path[k]] = 0.0;
    double key = 0.0;
    unsigned long long rank = RANK_NONE;
    if (forced_q < 0) fold_candidates<RULE>(lp.cand_j, lp.cand_key, n_price_blocks, tid, NET_THREADS, key, rank);
    int block = 0;
    const int winner = entering_winner<RULE>(key, rank, s_key, s_rank, block);
    if (tid != 0) return;
    int q = -1;
    double cbar = 0.0;
    if (forced_q >= 0) {
        q = forced_q;
        double cb = reduced_cost_of(lp.cost[q], lp.col_start, lp.row_index, lp.value, lp.minus_pi, q);
        if (lp.ub && lp.flipped[q]) cb = -cb;
        cbar = cb;
    } else if (winner >= 0) {
        q = winner;
        cbar = lp.cand_cbar[block];
    }
    if (q < 0) {
        ctl_no_entering(*ctl, mode);
        t.state[1] = 0;
        return;
    }
    const int e0 = lp.col_start[q], len = lp.col_start[q + 1] - e0;  // (0: an arc between two removed vertices, alpha = 0)
    const int u = len > 0 ? lp.row_index[e0] : -1, v = len > 1 ? lp.row_index[e0 + 1] : -1;
    const double au = len > 0 ? lp.value[e0] : 0.0, av = len > 1 ? lp.value[e0 + 1] : 0.0;
    const int stamp = t.state[0] + 1;
    t.state[0] = stamp;
    int nu = 0;
    for (int x = u; x >= 0 && nu < m; x = t.parent[x]) {
        t.mark[x] = stamp;
        t.chain[nu++] = x;
    }
    int common = -1, n_path = 0, steps = 0;
    for (int x = v; x >= 0 && steps < m; x = t.parent[x], ++steps) {
        if (t.mark[x] == stamp) {
            common = x;
            break;
        }
        const int s = t.slot[x];
        lp.alpha_in[s] = (double)t.sign[x] * av;
        t.path[n_path++] = s;
    }
    for (int k = 0; k < nu && n_path < m; ++k) {
        const int x = t.chain[k];
        if (x == common) break;
        const int s = t.slot[x];
        lp.alpha_in[s] = (double)t.sign[x] * au;
        t.path[n_path++] = s;
    }
    t.state[1] = n_path;
    ctl->q = q;
    ctl->cbar_q = cbar;
}

// ---------------------------------------------------------------------------------------------------
// After the ratio test of a basis change (status running, pending): for every row j, in the forest BEFORE the pivot,
//   w_j   = (B^-T alpha)_j = sum over the arcs of j's root path of alpha[slot] sign       (Goldfarb-Reid update of the next pass)
//   rho_j = row p of the new inverse = sign[child[p]] / alpha_pq when j lies below the leaving arc, else 0
//   -pi_j -= cbar_q rho_j                                                                  (the constant shift on that subtree)
// the same values the explicit carry's update kernel writes (every one an integer: exact).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NET_THREADS) net_update_kernel(DeviceLP lp, NetTree t) {
    const Ctl* ctl = lp.ctl;
    const int m = lp.m;
    const int j = blockIdx.x * NET_THREADS + threadIdx.x;
    const int status = ctl->status, pending = ctl->pending, p = ctl->p, rho_buf = ctl->rho_buf;
    const double alpha_pq = ctl->alpha_pq, cbar_q = ctl->cbar_q;
    if (status != ST_RUNNING || !pending) return;
    const int below = t.child[p];
    double w = 0.0;
    bool inside = false;
    int steps = 0;
    if (j < m)
        for (int x = j; x >= 0 && steps < m; x = t.parent[x], ++steps) {
            w += lp.alpha[t.slot[x]] * (double)t.sign[x];
            inside |= x == below;
        }
    if (t.stats) {  // RELP_SW_NETWORK_STATS: row depths and the subtree size of this pivot, one atomic per wave
        unsigned long long in_count = inside ? 1 : 0, depth_sum = (unsigned long long)steps;
        int depth_max = steps;
        for (int d = NET_WAVE / 2; d > 0; d >>= 1) {
            in_count += __shfl_xor(in_count, d);
            depth_sum += __shfl_xor(depth_sum, d);
            depth_max = max(depth_max, __shfl_xor(depth_max, d));
        }
        if ((threadIdx.x & (NET_WAVE - 1)) == 0) {
            atomicAdd(t.stats + NS_SUBTREE_NOW, in_count);
            atomicAdd(t.stats + NS_DEPTH_SUM, depth_sum);
            atomicMax(t.stats + NS_DEPTH_MAX, (unsigned long long)depth_max);
        }
    }
    if (j >= m) return;
    const double r = inside ? (double)t.sign[below] / alpha_pq : 0.0;
    lp.w[j] = w;
    lp.rho[j] = r;
    double pi = lp.minus_pi[j];
    if (r != 0.0) {
        pi -= cbar_q * r;
        lp.minus_pi[j] = pi;
    }
    if (lp.prw) {
        lp.prw[(size_t)4 * j] = pi;
        lp.prw[(size_t)4 * j + 1] = r;
        lp.prw[(size_t)4 * j + 2] = w;
    }
    mark_rho_row(lp, rho_buf, j, r);
}

// The forest after the basis change: the entering arc hangs the endpoint below the leaving arc onto the other endpoint (or onto the
// virtual root: a single-entry column), and the parent pointers on the path from that endpoint up to the leaving arc are reversed.
__global__ void net_rehang_kernel(DeviceLP lp, NetTree t) {
    const Ctl* ctl = lp.ctl;
    if (ctl->status != ST_RUNNING || !ctl->pending) return;
    const int m = lp.m, p = ctl->p, q = ctl->q;
    if (t.stats) {  // (net_update_kernel has counted the rows below the leaving arc)
        const unsigned long long size = t.stats[NS_SUBTREE_NOW];
        t.stats[NS_PIVOTS] += 1;
        t.stats[NS_SUBTREE_SUM] += size;
        t.stats[NS_SUBTREE_MAX] = max(t.stats[NS_SUBTREE_MAX], size);
        t.stats[NS_SUBTREE_NOW] = 0;
        const unsigned long long path = (unsigned long long)t.state[1];  // (the path net_ftran_kernel found for this pivot)
        t.stats[NS_PATH_SUM] += path;
        t.stats[NS_PATH_MAX] = max(t.stats[NS_PATH_MAX], path);
    }
    const int below = t.child[p];
    const int e0 = lp.col_start[q], len = lp.col_start[q + 1] - e0;
    const int u = lp.row_index[e0], v = len > 1 ? lp.row_index[e0 + 1] : -1;
    const double au = lp.value[e0], av = len > 1 ? lp.value[e0 + 1] : 0.0;
    const double sgn_q = (lp.ub && lp.flipped[q]) ? -1.0 : 1.0;
    bool u_below = len == 1;
    int steps = 0;
    for (int x = u; !u_below && x >= 0 && steps < m; x = t.parent[x], ++steps) u_below = x == below;
    const int e = u_below ? u : v, f = u_below ? v : u;
    int prev_node = f, prev_slot = p;
    signed char prev_sign = (signed char)(sgn_q * (u_below ? au : av));
    steps = 0;
    for (int x = e; x >= 0 && steps <= m; ++steps) {
        const int next = t.parent[x], old_slot = t.slot[x];
        const signed char old_sign = t.sign[x];
        t.parent[x] = prev_node;
        t.slot[x] = prev_slot;
        t.sign[x] = prev_sign;
        t.child[prev_slot] = x;
        if (x == below) break;
        prev_node = x;
        prev_slot = old_slot;
        prev_sign = (signed char)-old_sign;  // (an incidence column: the other end carries the opposite sign)
        x = next;
    }
}

// -pi_j = -sum over j's root path of c_B[slot] sign (c_B and the objective from cb_kernel)
__global__ void __launch_bounds__(NET_THREADS) net_pi_kernel(DeviceLP lp, NetTree t) {
    const int m = lp.m;
    const int j = blockIdx.x * NET_THREADS + threadIdx.x;
    if (j >= m) return;
    double acc = 0.0;
    int steps = 0;
    for (int x = j; x >= 0 && steps < m; x = t.parent[x], ++steps) acc += lp.cb[t.slot[x]] * (double)t.sign[x];
    lp.minus_pi[j] = -acc;
    if (lp.prw) lp.prw[(size_t)4 * j] = -acc;
}

// row r of B^-1 (drive_out_artificials)
__global__ void __launch_bounds__(NET_THREADS) net_row_kernel(DeviceLP lp, NetTree t, int r, double* out) {
    const int m = lp.m;
    const int j = blockIdx.x * NET_THREADS + threadIdx.x;
    if (j >= m) return;
    const int below = t.child[r];
    bool inside = false;
    int steps = 0;
    for (int x = j; x >= 0 && steps < m && !inside; x = t.parent[x], ++steps) inside = x == below;
    out[j] = inside ? (double)t.sign[below] : 0.0;
}

namespace {
int net_grid(int m) { return (m + NET_THREADS - 1) / NET_THREADS; }
}  // namespace

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
void Solver::net_allocate() {
    const int m = d_.m;
    net_.parent = device_alloc<int>(m);
    net_.slot = device_alloc<int>(m);
    net_.sign = device_alloc<signed char>(m);
    net_.child = device_alloc<int>(m);
    net_.mark = device_alloc<int>(m);
    net_.chain = device_alloc<int>(m);
    net_.path = device_alloc<int>(m);
    net_.state = device_alloc<int>(2);
    if (opt_.switches & RELP_SW_NETWORK_STATS) {
        net_.stats = device_alloc<unsigned long long>(NS_WORDS);
        RELP_HIP(hipMemsetAsync(net_.stats, 0, NS_WORDS * sizeof(unsigned long long), stream_));
    }
    RELP_HIP(hipMemsetAsync(net_.mark, 0, (size_t)m * sizeof(int), stream_));
    RELP_HIP(hipMemsetAsync(net_.state, 0, 2 * sizeof(int), stream_));
    RELP_HIP(hipMemsetAsync(d_.alpha_in, 0, (size_t)m * sizeof(double), stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

// The forest of a basis (device slots -> device columns), breadth first from the root arcs.  `flipped` (implicit bounds; empty
// otherwise): complemented columns sit in B negated.
HostTree Solver::net_build(const std::vector<int>& basis, const std::vector<int>& flipped) const {
    const int m = d_.m;
    const std::vector<int>& cs = host_.col_start;
    const std::vector<int>& ri = host_.row_index;
    const std::vector<double>& va = host_.value;
    HostTree t;
    t.parent.assign(m, -1);
    t.slot.assign(m, -1);
    t.child.assign(m, -1);
    t.sign.assign(m, 0);
    t.depth.assign(m, 0);
    t.order.clear();
    t.order.reserve(m);
    std::vector<int> adj_start(m + 1, 0), adj;
    auto sgn = [&](int column) { return (!flipped.empty() && flipped[column]) ? -1 : 1; };
    for (int i = 0; i < m; ++i) {
        const int j = basis[i];
        if (cs[j + 1] - cs[j] == 2) {
            adj_start[ri[cs[j]] + 1]++;
            adj_start[ri[cs[j] + 1] + 1]++;
        }
    }
    for (int r = 0; r < m; ++r) adj_start[r + 1] += adj_start[r];
    adj.resize(adj_start[m]);
    {
        std::vector<int> fill(adj_start.begin(), adj_start.end() - 1);
        for (int i = 0; i < m; ++i) {
            const int j = basis[i];
            if (cs[j + 1] - cs[j] == 2) {
                adj[fill[ri[cs[j]]]++] = i;
                adj[fill[ri[cs[j] + 1]]++] = i;
            }
        }
    }
    for (int i = 0; i < m; ++i) {
        const int j = basis[i];
        if (cs[j + 1] - cs[j] != 1) continue;
        const int r = ri[cs[j]];
        if (t.slot[r] >= 0) throw std::runtime_error("RELP_CARRY_NETWORK: the basis is not a spanning forest (two root arcs in one tree)");
        t.slot[r] = i;
        t.child[i] = r;
        t.sign[r] = (signed char)(va[cs[j]] * sgn(j));
        t.depth[r] = 1;
        t.order.push_back(r);
    }
    for (size_t head = 0; head < t.order.size(); ++head) {
        const int x = t.order[head];
        for (int a = adj_start[x]; a < adj_start[x + 1]; ++a) {
            const int i = adj[a];
            if (i == t.slot[x]) continue;
            const int j = basis[i];
            const int e = ri[cs[j]] == x ? cs[j] + 1 : cs[j];
            const int y = ri[e];
            if (t.slot[y] >= 0) throw std::runtime_error("RELP_CARRY_NETWORK: the basis is not a spanning forest (a cycle)");
            t.parent[y] = x;
            t.slot[y] = i;
            t.child[i] = y;
            t.sign[y] = (signed char)(va[e] * sgn(j));
            t.depth[y] = t.depth[x] + 1;
            t.order.push_back(y);
        }
    }
    if ((int)t.order.size() != m) throw std::runtime_error("RELP_CARRY_NETWORK: the basis is not a spanning forest (a tree without a root arc)");
    return t;
}

void Solver::net_upload(const HostTree& t) {
    RELP_HIP(hipMemcpyAsync(net_.parent, t.parent.data(), t.parent.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(net_.slot, t.slot.data(), t.slot.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(net_.child, t.child.data(), t.child.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(net_.sign, t.sign.data(), t.sign.size(), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

HostTree Solver::net_download() {
    const int m = d_.m;
    std::vector<int> basis(m), flipped;
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    if (path_.bounded) {
        flipped.resize(d_.n);
        RELP_HIP(hipMemcpyAsync(flipped.data(), d_.flipped, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    }
    RELP_HIP(hipStreamSynchronize(stream_));
    for (int i = 0; i < m; ++i)
        if (basis[i] < 0 || basis[i] >= d_.n) throw std::runtime_error("the device returned an invalid basis");
    return net_build(basis, flipped);  // (the same forest the device keeps, rebuilt from its basis)
}

void Solver::net_refresh(bool xb, bool pi) {
    const int m = d_.m;
    if (xb) {  // x_B = B^-1 rhs from the leaves up, in the forest's breadth-first order: the same sums in the same order every time
        const HostTree t = net_download();
        std::vector<double> below(m), x(m);
        RELP_HIP(hipMemcpyAsync(below.data(), d_.rhs, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        for (int k = m - 1; k >= 0; --k) {
            const int r = t.order[k];
            x[t.slot[r]] = t.sign[r] * below[r];
            if (t.parent[r] >= 0) below[t.parent[r]] += below[r];
        }
        RELP_HIP(hipMemcpyAsync(d_.xB, x.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    if (pi) {
        launch_cb(d_, stream_);  // c_B and -obj = -c_B' x_B
        hipLaunchKernelGGL(net_pi_kernel, dim3(net_grid(m)), dim3(NET_THREADS), 0, stream_, d_, net_);
    }
}

// gamma_j = 1 + |B^-1 a_j|^2 = 1 + (arcs on the tree path of column j)
void Solver::net_gamma(const HostTree& t, const std::vector<int>& pos, std::vector<double>* gamma) const {
    const int n = d_.n, n_art = d_.n_art;
    gamma->assign(n, 1.0);
    const std::vector<int>& cs = host_.col_start;
    const std::vector<int>& ri = host_.row_index;
    auto range = [&](int first, int last) {
        for (int j = first; j < last; ++j) {
            if (pos[j] >= 0) continue;
            int len = 0;
            if (cs[j + 1] == cs[j]) {
            } else if (cs[j + 1] - cs[j] == 1) {
                len = t.depth[ri[cs[j]]];
            } else {
                int a = ri[cs[j]], b = ri[cs[j] + 1];
                while (a >= 0 && b >= 0 && a != b) {
                    if (t.depth[a] >= t.depth[b]) { a = t.parent[a]; ++len; }
                    else { b = t.parent[b]; ++len; }
                }
                if (a != b) {  // two trees: both root paths
                    for (; a >= 0; a = t.parent[a]) ++len;
                    for (; b >= 0; b = t.parent[b]) ++len;
                }
            }
            (*gamma)[j] = 1.0 + len;
        }
    };
    const int n_threads = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    const int columns = n - n_art;
    if (n_threads <= 1 || columns < 65536) {
        range(n_art, n);
    } else {
        std::vector<std::thread> pool;
        const int chunk = (columns + n_threads - 1) / n_threads;
        for (int k = 0; k < n_threads; ++k) {
            const int first = n_art + k * chunk, last = std::min(n, first + chunk);
            if (first < last) pool.emplace_back(range, first, last);
        }
        for (auto& th : pool) th.join();
    }
}

void Solver::net_set_gamma() {
    std::vector<int> pos(d_.n);
    RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    const HostTree t = net_download();
    std::vector<double> gamma;
    net_gamma(t, pos, &gamma);
    RELP_HIP(hipMemcpyAsync(d_.gamma, gamma.data(), gamma.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

// The crash basis of crash_basis() handed to the forest: x_B from the tree (leaves up), the weights from path lengths.  Kept only
// when primal feasible, as the explicit carry's.
bool Solver::net_crash(const std::vector<int>& basis) {
    const int m = d_.m, n = d_.n;
    const HostTree t = net_build(basis, std::vector<int>());  // (nothing is complemented at the start of phase one)
    std::vector<double> sub(host_.rhs.begin(), host_.rhs.end()), xb(m, 0.0);
    for (int k = m - 1; k >= 0; --k) {
        const int x = t.order[k];
        xb[t.slot[x]] = t.sign[x] * sub[x];
        if (t.parent[x] >= 0) sub[t.parent[x]] += sub[x];
    }
    std::vector<double> ub;
    if (path_.bounded) {
        ub.resize(n);
        RELP_HIP(hipMemcpyAsync(ub.data(), d_.ub, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    double scale = 1.0;
    for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(host_.rhs[i]));
    for (int i = 0; i < m; ++i) {
        if (xb[i] < -1e-9 * scale) return false;
        if (path_.bounded && xb[i] > ub[basis[i]] + 1e-9 * scale) return false;
        if (xb[i] < 0.0) xb[i] = 0.0;
    }
    std::vector<int> pos(n, -1);
    if (path_.bounded)
        for (int j = d_.n_art; j < n; ++j)
            if (zero_width_[j]) pos[j] = -3;
    for (int i = 0; i < m; ++i) pos[basis[i]] = i;
    std::vector<double> gamma(n, 1.0);
    if (opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE) net_gamma(t, pos, &gamma);
    net_upload(t);
    RELP_HIP(hipMemcpyAsync(d_.basis, basis.data(), m * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_.pos, pos.data(), n * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_.xB, xb.data(), m * sizeof(double), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_.gamma, gamma.data(), n * sizeof(double), hipMemcpyHostToDevice, stream_));
    if (path_.bounded) {
        std::vector<double> xub(m);
        for (int i = 0; i < m; ++i) xub[i] = ub[basis[i]];
        RELP_HIP(hipMemcpyAsync(d_.xub, xub.data(), m * sizeof(double), hipMemcpyHostToDevice, stream_));
    }
    RELP_HIP(hipStreamSynchronize(stream_));
    binv_identity_ = false;
    gamma_ready_ = opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE;
    return true;
}

void launch_net_row(const DeviceLP& d, const NetTree& t, int r, double* out, hipStream_t s) {
    hipLaunchKernelGGL(net_row_kernel, dim3(net_grid(d.m)), dim3(NET_THREADS), 0, s, d, t, r, out);
}

// parts: 1 entering column, path and ratio test; 2 the forest update (mode 0)
void Solver::net_enqueue_pivot(int mode, int parts) {
    const int slots = path_.slots();
    const int skip_art = phase_ == 2 ? 1 : 0;
    if (parts & 1) {
        if (opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE)
            hipLaunchKernelGGL(net_ftran_kernel<RELP_PIVOT_STEEPEST_EDGE>, dim3(1), dim3(NET_THREADS), 0, stream_, d_, net_, slots, mode);
        else
            hipLaunchKernelGGL(net_ftran_kernel<RELP_PIVOT_DANTZIG>, dim3(1), dim3(NET_THREADS), 0, stream_, d_, net_, slots, mode);
        if (!path_.multi_workgroup_ratio) {
            launch_ftran_ratio(d_, path_, opt_.pivot_rule, opt_.tol_pivot, ratio_delta(), skip_art, mode, 1, stream_);
        } else {
            if (mode != 0) throw std::invalid_argument("RELP_CARRY_NETWORK: the ratio test without a basis change is implemented up to 8192 rows");
            // Every non-zero of alpha is +-1 on a network basis, so the two-pass test with a slack of 0 IS the reference's rule: pass 1
            // finds the exact minimum ratio, pass 2 takes, among the rows that reach it, the largest |alpha| (all 1) and then the lowest
            // leaving column (Bland) -- the textbook rule of the register-resident kernel, at any number of rows.
            launch_k2l_preselected(d_, opt_.tol_pivot, path_.ratio_textbook ? 0.0 : opt_.harris_delta, skip_art, stream_);
        }
    }
    if (mode != 0 || !(parts & 2)) return;
    hipLaunchKernelGGL(net_update_kernel, dim3(net_grid(d_.m)), dim3(NET_THREADS), 0, stream_, d_, net_);
    hipLaunchKernelGGL(net_rehang_kernel, dim3(1), dim3(1), 0, stream_, d_, net_);
}

// ---------------------------------------------------------------------------------------------------
// Exact certificate from the forest (certify = 1, finite optimum): with implicit bounds the right-hand side is b minus u_j a_j of
// every complemented column, x_B is accumulated from the leaves up and pi from the roots down, all in exact rationals; every basic
// variable must lie within its bounds and every reduced cost have the sign of its bound.  O(m + n) memory.
// ---------------------------------------------------------------------------------------------------
void Solver::net_certify(relp_result* result) {
    const double t0 = now_seconds_net();
    const int m = d_.m, n = d_.n, n_art = d_.n_art;
    const MatrixData& md = form_.data;
    std::string message;
    bool ok = false;
    try {
        std::vector<int> basis(m), pos(n), flipped;
        RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        if (path_.bounded) {
            flipped.resize(n);
            RELP_HIP(hipMemcpyAsync(flipped.data(), d_.flipped, n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        }
        RELP_HIP(hipStreamSynchronize(stream_));
        const HostTree t = net_build(basis, flipped);
        // exact data of the device LP: column j's entries are +-1 (checked at load), costs and bounds from the model
        auto cost = [&](int j) { return j < n_art ? Rat(0) : md.cost_value(j - n_art); };
        std::vector<Rat> upper(n);
        std::vector<char> has_upper(n, 0);
        if (path_.bounded) {
            for (int j = 0; j < md.nr_normal_variables(); ++j)
                if (md.variables[j].has_upper) { has_upper[n_art + j] = 1; upper[n_art + j] = md.variables[j].upper; }
            for (int k = 0; k < md.nr_range; ++k) { has_upper[n_art + md.col_end[0] + k] = 1; upper[n_art + md.col_end[0] + k] = md.ranges[k]; }
        }
        const std::vector<Rat> b_exact = md.right_hand_side();
        std::vector<Rat> rhs(b_exact.begin(), b_exact.begin() + m);
        // every complemented column, basic or not, moves u_j a_j to the right-hand side (as the device and set_basis hold it: a
        // column keeps its complemented form when it enters the basis, and its basic value is then u_j - x_j)
        for (int j = n_art; j < n; ++j)
            if (path_.bounded && flipped[j])
                for (int e = host_.col_start[j]; e < host_.col_start[j + 1]; ++e) rhs[host_.row_index[e]] = rhs[host_.row_index[e]] - upper[j] * Rat((long long)host_.value[e]);
        // x_B in B's own (possibly complemented) orientation: x_B[slot] = sign * (sum of rhs below)
        std::vector<Rat> below(rhs), xb(m);
        for (int k = m - 1; k >= 0; --k) {
            const int x = t.order[k];
            xb[t.slot[x]] = t.sign[x] < 0 ? -below[x] : below[x];
            if (t.parent[x] >= 0) below[t.parent[x]] = below[t.parent[x]] + below[x];
        }
        // y = B^-T c_B from the roots down: y_x = y_parent + c_B[slot] sign
        std::vector<Rat> y(m);
        for (int k = 0; k < m; ++k) {
            const int x = t.order[k];
            const int j = basis[t.slot[x]];
            Rat c = cost(j);
            if (path_.bounded && flipped[j]) c = -c;
            const Rat term = t.sign[x] < 0 ? -c : c;
            y[x] = (t.parent[x] >= 0 ? y[t.parent[x]] : Rat(0)) + term;
        }
        // the values of the provider columns and the checks
        std::vector<int> columns;
        std::vector<Rat> values;
        Rat objective = form_.fixed_cost;
        bool feasible = true, optimal = true;
        int bad = -1;
        for (int i = 0; i < m && feasible; ++i) {
            const int j = basis[i];
            Rat v = xb[i];
            if (v.sign() < 0) { feasible = false; bad = j; break; }
            if (j < n_art) {
                if (!v.is_zero()) { feasible = false; bad = j; }
                continue;
            }
            if (path_.bounded && has_upper[j]) {
                if (upper[j] < v) { feasible = false; bad = j; break; }
                if (flipped[j]) v = upper[j] - v;
            }
            objective = objective + md.cost_value(j - n_art) * v;
            if (!v.is_zero()) { columns.push_back(j - n_art); values.push_back(v); }
        }
        for (int j = n_art; j < n && feasible && optimal; ++j) {
            if (pos[j] >= 0) continue;
            Rat d = cost(j);
            for (int e = host_.col_start[j]; e < host_.col_start[j + 1]; ++e) d = d - Rat((long long)host_.value[e]) * y[host_.row_index[e]];
            const bool up = path_.bounded && flipped[j];
            if (up) {
                objective = objective + md.cost_value(j - n_art) * upper[j];
                if (!upper[j].is_zero()) { columns.push_back(j - n_art); values.push_back(upper[j]); }
            }
            if (pos[j] == -3) continue;  // fixed: either sign
            if (up ? d.sign() > 0 : d.sign() < 0) { optimal = false; bad = j; }
        }
        if (!feasible) message = "network certificate: the basic solution is infeasible at column " + std::to_string(bad);
        else if (!optimal) message = "network certificate: column " + std::to_string(bad) + " has a reduced cost of the wrong sign";
        else {
            ok = true;
            exact_objective = objective.d == 1 ? to_string128(objective.n) : to_string(objective);
            exact_primal = make_exact_primal(columns, values);
        }
    } catch (const RatOverflow& e) {
        message = std::string("network certificate: ") + e.what();
    }
    result->certified = ok ? 1 : 0;
    result->exact_repair_pivots = 0;
    result->certify_seconds = now_seconds_net() - t0;
    if (!ok) last_error = message;
}

// The fine-grained FTRAN / BTRAN on the host: B^-1 v from the leaves up, v' B^-1 from the roots down.
std::vector<double> Solver::net_host_solve(const HostTree& t, bool transposed, const std::vector<double>& v) const {
    const int m = d_.m;
    std::vector<double> out(m, 0.0);
    if (!transposed) {
        std::vector<double> below(v);
        for (int k = m - 1; k >= 0; --k) {
            const int x = t.order[k];
            out[t.slot[x]] = t.sign[x] * below[x];
            if (t.parent[x] >= 0) below[t.parent[x]] += below[x];
        }
    } else {
        for (int k = 0; k < m; ++k) {
            const int x = t.order[k];
            out[x] = (t.parent[x] >= 0 ? out[t.parent[x]] : 0.0) + v[t.slot[x]] * t.sign[x];
        }
    }
    return out;
}

}  // namespace relp
