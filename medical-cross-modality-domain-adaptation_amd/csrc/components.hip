// Connected components of a label volume and the "keep the largest" filter: uint8 labels [D0, D1, D2], C order (D2
// fastest), n = D0 D1 D2 < 2^31.  A component = a maximal set of voxels of ONE non-zero label < ncls joined by steps of the 6 / 18 / 26
// neighbourhood (connectivity 1 / 2 / 3); roots[v] = the smallest flat index of v's component, -1 for background.  Everything is integer.
//
// Labelling is union-find over one int32 parent array in the workspace, three launches whatever the data:
//   cc_tile_kernel     one workgroup per 8 x 8 x 32 tile (z fastest, like the memory; 2 048 voxels, 8 per lane: lane -> (y, z), the lane's
//                      k-th voxel is x = k).  Labels and parents live in LDS under tile-local indices, which order voxels exactly as their
//                      flat indices do.  A z row is half a wave: the run of equal labels a voxel lies in comes from one ballot, and the
//                      voxel starts out linked to the run's first voxel; the other backward neighbours (x - 1, y - 1, and the diagonals of
//                      connectivity 2 and 3) are merged with the lock-free union below on LDS atomics.  __syncthreads only.  Then every
//                      voxel's tile root, as a flat index, goes to parent[] (-1 for background): plain stores, read by the NEXT launch.
//   cc_border_kernel   the same workgroup -> tile map; a voxel whose backward neighbour lies in another tile and carries its label merges
//                      the two trees in parent[].
//   cc_flatten_kernel  roots[v] = find(v): parent[] is read-only in this launch, roots is a different allocation.
//
// The union (uf_union): find both roots, atomicMin the LARGER root's entry with the smaller one; when the value that comes back is not the
// larger root itself, somebody else linked it first — carry on from that value (it is in the same component and smaller).
//   * Links only ever point to a smaller index and an entry only ever decreases, so a tree's root is the smallest index of its set: the
//     representative does not depend on the schedule, and the output is bit-identical from run to run.
//   * Cross-XCD visibility: the per-XCD L2s are not coherent for plain accesses inside one launch.  In cc_border_kernel parent[] is
//     WRITTEN only by atomicMin (performed at the device-coherent level) and READ only by relaxed agent-scope atomic loads (they bypass the
//     CU's L1).  A stale read is harmless: every value an entry ever held is a member of the same component and no smaller than the
//     current one, so following it stays inside the component, and the atomicMin that ends an attempt returns the true current value,
//     from which the loop continues.  Only cc_flatten_kernel, the next launch, relies on everything being visible.
//   * Termination: find walks strictly downwards (< n steps); every round of the union replaces the larger of its two indices by a
//     strictly smaller one (< n rounds).  Nobody waits for anybody: no flags, no tickets, no barrier across workgroups.  Each loop still
//     carries the cap n; reaching it adds to the error counter at the head of the workspace and ends the lane's work.
//
// Filtering: cc_count_kernel sums component sizes at the root's slot of an int32 array in the workspace — a lane walks 16 consecutive
// voxels as runs of equal roots, a workgroup merges its runs in an LDS table keyed by the root and then issues one global add per root it
// met: ONE atomic add for 4 096 voxels inside a structure.  cc_rank_kernel (one launch per rank, max(keep, 1) launches) finds per class the largest key (size << 32 | ~root) below the
// previous rank's: ties go to the lower root.  cc_apply_kernel writes the filtered labels (out may be vol: a lane reads and writes its own
// voxel only) and cc_stats_kernel writes the int64 rows.  Integer atomics only: exact in any order.
//
// Hole filling (pnp_fill_holes) labels the BACKGROUND with the same three launches and counts its components' sizes with
// cc_count_kernel; its own kernels (fh_*) stand further down, before the entry points.
#include "pnp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxExtent = 4096;
constexpr int kMaxKeep = 8;
constexpr int T0 = 8, T1 = 8, T2 = 32;     // tile extents; T2 = half a wave, T1 * T2 = the workgroup
constexpr int kTile = T0 * T1 * T2;
constexpr int kRun = 16;                   // consecutive voxels per lane of cc_count_kernel
constexpr int kSlotBits = 10, kSlots = 1 << kSlotBits, kProbes = 8;       // its LDS table
constexpr size_t kHeaderBytes = 1024;

struct Header {                            // the first kHeaderBytes of the workspace
    unsigned int err_label;                // loops of the labelling that reached their cap (zeroed by pnp_label_components)
    unsigned int err_filter;               // lanes of the filter that met a roots entry >= n (zeroed by pnp_filter_components, like all below)
    unsigned int pad[62];
    unsigned long long best[MAXC][kMaxKeep];       // key of the rank-th largest component per class, 0 = none
    unsigned long long found[MAXC], kept[MAXC];       // found = (components << 32) + voxels
};
static_assert(sizeof(Header) <= kHeaderBytes, "header");

// the backward half of the 26-neighbourhood (lexicographically negative offsets), sorted by the number of non-zero entries:
// connectivity 1 takes the first 3, 2 the first 9, 3 all 13
__constant__ signed char kOff[13][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1},
                                        {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},
                                        {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};
constexpr int kOffZ = 2;                   // (0, 0, -1): inside a tile the ballot has done it

template <int SCOPE>
__device__ __forceinline__ int uf_find(int* par, int x, int cap, bool& over) {
    for (int i = 0; i < cap; ++i) {
        const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;                             // p < x
    }
    over = true;
    return x;
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(int* par, int a, int b, int cap, bool& over) {
    for (int i = 0; i < cap; ++i) {
        a = uf_find<SCOPE>(par, a, cap, over);
        b = uf_find<SCOPE>(par, b, cap, over);
        if (over || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;              // a was a root and now points to b
        a = old;                           // old < a: a had been linked meanwhile (the entry now holds min(old, b)); join old and b
    }
    over = true;
}

struct Dims {
    int D0, D1, D2, nt1, nt2;
};

__device__ __forceinline__ void tile_origin(const Dims& d, int& x0, int& y0, int& z0) {
    const int b = blockIdx.x;
    const int bz = b % d.nt2, bxy = b / d.nt2;
    x0 = (bxy / d.nt1) * T0;
    y0 = (bxy % d.nt1) * T1;
    z0 = bz * T2;
}

__global__ void __launch_bounds__(kThreads) cc_tile_kernel(const unsigned char* __restrict__ vol, int* __restrict__ parent, Header* h,
                                                           const Dims d, int ncls, int noff) {
    __shared__ int par[kTile];
    __shared__ unsigned char lab[kTile];
    int x0, y0, z0;
    tile_origin(d, x0, y0, z0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int ly = tid >> 5, lz = tid & 31;
    const int gy = y0 + ly, gz = z0 + lz;
    const bool col = gy < d.D1 && gz < d.D2;
#pragma unroll
    for (int k = 0; k < T0; ++k) {
        const int gx = x0 + k;
        unsigned char l = 0;
        if (col && gx < d.D0) {
            l = vol[(gx * d.D1 + gy) * d.D2 + gz];
            if (l >= ncls) l = 0;
        }
        // the z run: bit `lane` = "continues its left neighbour"; the run starts at the highest clear bit at or below the lane (lz = 0 never continues)
        const unsigned char left = (unsigned char)__shfl_up((int)l, 1);
        const unsigned long long cont = __ballot(lz > 0 && l != 0 && l == left);
        const unsigned long long upto = (~cont) & (~0ull >> (63 - lane));
        const int start = 63 - __clzll((long long)upto);
        const int t = k * kThreads + tid;
        lab[t] = l;
        par[t] = t - (lane - start);
    }
    __syncthreads();
    bool over = false;
    for (int k = 0; k < T0; ++k) {
        const int t = k * kThreads + tid;
        const unsigned char l = lab[t];
        if (l == 0) continue;
        for (int j = 0; j < noff; ++j) {
            if (j == kOffZ) continue;
            const int nx = k + kOff[j][0], ny = ly + kOff[j][1], nz = lz + kOff[j][2];
            if (nx < 0 || ny < 0 || ny >= T1 || nz < 0 || nz >= T2) continue;
            const int u = (nx * T1 + ny) * T2 + nz;
            if (lab[u] == l) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, t, u, kTile, over);
            if (over) break;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < T0; ++k) {
        const int gx = x0 + k;
        if (!(col && gx < d.D0)) continue;
        const int t = k * kThreads + tid;
        int g = -1;
        if (lab[t] != 0) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, t, kTile, over);
            g = ((x0 + r / (T1 * T2)) * d.D1 + y0 + (r / T2) % T1) * d.D2 + z0 + r % T2;
        }
        parent[(gx * d.D1 + gy) * d.D2 + gz] = g;
    }
    if (over) atomicAdd(&h->err_label, 1u);
}

__global__ void __launch_bounds__(kThreads) cc_border_kernel(const unsigned char* __restrict__ vol, int* parent, Header* h, const Dims d,
                                                             int ncls, int noff, int n) {
    int x0, y0, z0;
    tile_origin(d, x0, y0, z0);
    const int tid = threadIdx.x;
    const int ly = tid >> 5, lz = tid & 31;
    const int gy = y0 + ly, gz = z0 + lz;
    if (gy >= d.D1 || gz >= d.D2) return;
    bool over = false;
    for (int k = 0; k < T0; ++k) {
        const int gx = x0 + k;
        if (gx >= d.D0) break;
        if (k > 0 && ly > 0 && ly < T1 - 1 && lz > 0 && lz < T2 - 1) continue;       // no backward neighbour outside the tile
        const int v = (gx * d.D1 + gy) * d.D2 + gz;
        const unsigned char l = vol[v];
        if (l == 0 || l >= ncls) continue;
        for (int j = 0; j < noff; ++j) {
            const int dx = kOff[j][0], dy = kOff[j][1], dz = kOff[j][2];
            const bool inside = k + dx >= 0 && ly + dy >= 0 && ly + dy < T1 && lz + dz >= 0 && lz + dz < T2;
            if (inside) continue;
            const int nx = gx + dx, ny = gy + dy, nz = gz + dz;
            if (nx < 0 || ny < 0 || ny >= d.D1 || nz < 0 || nz >= d.D2) continue;
            const int u = (nx * d.D1 + ny) * d.D2 + nz;
            if (vol[u] == l) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, v, u, n, over);
            if (over) break;
        }
        if (over) break;
    }
    if (over) atomicAdd(&h->err_label, 1u);
}

__global__ void __launch_bounds__(kThreads) cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ roots, Header* h, int n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int x = parent[i];
    if (x >= 0) {
        int steps = 0;
        for (int p = parent[x]; p != x; p = parent[x]) {
            x = p;
            if (++steps >= n) {
                atomicAdd(&h->err_label, 1u);
                break;
            }
        }
    }
    roots[i] = x;
}

// A workgroup covers kThreads * kRun consecutive voxels, a lane kRun consecutive ones (four 16-byte loads): the lane walks them as runs of
// equal roots and adds each finished run to a table in LDS keyed by the root (open addressing, kProbes probes, LDS atomics); a run that
// finds the table crowded goes straight to memory.  The table is then flushed with one global add per occupied slot: a workgroup inside
// one structure issues ONE global atomic for 4 096 voxels, and the global adds of a workgroup go to distinct addresses.
__device__ __forceinline__ void count_run(int* hkey, int* hcnt, int* sizes, int root, int cnt) {
    unsigned int s = ((unsigned int)root * 2654435761u) >> (32 - kSlotBits);
    for (int probe = 0; probe < kProbes; ++probe) {
        const int prev = atomicCAS(&hkey[s], -1, root);
        if (prev == -1 || prev == root) {
            atomicAdd(&hcnt[s], cnt);
            return;
        }
        s = (s + 1u) & (kSlots - 1);
    }
    atomicAdd(&sizes[root], cnt);
}

__global__ void __launch_bounds__(kThreads) cc_count_kernel(const int* __restrict__ roots, int* sizes, Header* h, int n) {
    __shared__ int hkey[kSlots];
    __shared__ int hcnt[kSlots];
    for (int s = threadIdx.x; s < kSlots; s += kThreads) {
        hkey[s] = -1;
        hcnt[s] = 0;
    }
    __syncthreads();
    const long long v0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kRun;
    int r[kRun];
    if (v0 + kRun <= n) {
        const int4* src = (const int4*)(roots + v0);          // 64-byte aligned: v0 is a multiple of 16
#pragma unroll
        for (int q = 0; q < kRun / 4; ++q) {
            const int4 t = src[q];
            r[4 * q + 0] = t.x;
            r[4 * q + 1] = t.y;
            r[4 * q + 2] = t.z;
            r[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRun; ++k) r[k] = v0 + k < n ? roots[v0 + k] : -1;
    }
    int cur = -1, cnt = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        int x = r[k];
        if (x >= n) {
            bad = true;
            x = -1;
        }
        if (x != cur) {
            if (cur >= 0) count_run(hkey, hcnt, sizes, cur, cnt);
            cur = x;
            cnt = 0;
        }
        ++cnt;
    }
    if (cur >= 0) count_run(hkey, hcnt, sizes, cur, cnt);
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots; s += kThreads)
        if (hkey[s] >= 0) atomicAdd(&sizes[hkey[s]], hcnt[s]);
    if (bad) atomicAdd(&h->err_filter, 1u);
}

__device__ __forceinline__ unsigned long long key_of(int size, int root) {
    return ((unsigned long long)(unsigned int)size << 32) | (unsigned int)~root;
}

// rank 0: every class's component count, voxel count and largest key; rank k > 0: per masked class the largest key below rank k - 1's.
// Only roots take part: their lanes merge in LDS, then one lane per class the workgroup met makes the global atomics.  found[c] packs
// (components << 32) + voxels: both stay below 2^31.  best[][] only grows, so a key no larger than the value read needs no atomic (a stale
// read is smaller and costs a needless atomic, never a missing one).
__global__ void __launch_bounds__(kThreads) cc_rank_kernel(const unsigned char* __restrict__ vol, const int* __restrict__ roots,
                                                           const int* __restrict__ sizes, Header* h, int n, int ncls, unsigned int mask,
                                                           int rank) {
    __shared__ unsigned long long s_best[MAXC], s_found[MAXC];
    if (threadIdx.x < MAXC) s_best[threadIdx.x] = s_found[threadIdx.x] = 0ull;
    __syncthreads();
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v < n && roots[v] == (int)v) {
        const unsigned char l = vol[v];
        if (l >= 1 && l < ncls) {
            const int s = sizes[v];
            const unsigned long long key = key_of(s, (int)v);
            if (rank == 0) {
                atomicMax(&s_best[l], key);
                atomicAdd(&s_found[l], (1ull << 32) + (unsigned long long)(unsigned int)s);
            } else if (((mask >> l) & 1u) && key < h->best[l][rank - 1]) {
                atomicMax(&s_best[l], key);
            }
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= 1 && c < ncls && s_best[c] != 0ull) {
        if (s_best[c] > __hip_atomic_load(&h->best[c][rank], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&h->best[c][rank], s_best[c]);
        if (rank == 0) atomicAdd(&h->found[c], s_found[c]);
    }
}

__global__ void __launch_bounds__(kThreads) cc_apply_kernel(const unsigned char* vol, const int* __restrict__ roots,
                                                            const int* __restrict__ sizes, unsigned char* out, Header* h, int n, int ncls,
                                                            unsigned int mask, int keep, long long min_size) {
    __shared__ unsigned long long s_kept[MAXC];
    if (threadIdx.x < MAXC) s_kept[threadIdx.x] = 0ull;
    __syncthreads();
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v < n) {
        unsigned char l = vol[v];
        if (l >= ncls) l = 0;
        const int r = roots[v];
        if (l != 0 && r >= 0 && r < n) {
            const int s = sizes[r];
            // a class outside the mask passes through whole
            const bool ok = !((mask >> l) & 1u) || ((long long)s >= min_size && (keep == 0 || key_of(s, r) >= h->best[l][keep - 1]));
            if (ok && r == (int)v) atomicAdd(&s_kept[l], (unsigned long long)(unsigned int)s);       // the root reports its component
            if (!ok) l = 0;
        }
        out[v] = l;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= 1 && c < ncls && s_kept[c] != 0ull) atomicAdd(&h->kept[c], s_kept[c]);
}

__global__ void cc_stats_kernel(const Header* __restrict__ h, long long* __restrict__ stats, int ncls) {
    const int c = threadIdx.x;
    if (c >= ncls) return;
    const bool on = c > 0;
    stats[4 * c + 0] = on ? (long long)(h->found[c] >> 32) : 0;
    stats[4 * c + 1] = on ? (long long)(h->found[c] & 0xffffffffull) : 0;
    stats[4 * c + 2] = on ? (long long)h->kept[c] : 0;
    stats[4 * c + 3] = on ? (long long)(h->best[c][0] >> 32) : 0;
}

// the extents both entry points and the query accept; *n = D0 D1 D2
bool dims_ok(int64_t D0, int64_t D1, int64_t D2, long long* n) {
    if (D0 < 1 || D1 < 1 || D2 < 1 || D0 > kMaxExtent || D1 > kMaxExtent || D2 > kMaxExtent) return false;
    *n = (long long)D0 * D1 * D2;
    return *n < (1ll << 31);
}

int check_dims(const char* who, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, long long* n) {
    PNP_REQUIRE(D0 >= 1 && D1 >= 1 && D2 >= 1 && D0 <= kMaxExtent && D1 <= kMaxExtent && D2 <= kMaxExtent,
                "%s: extents %lld x %lld x %lld outside [1, %d]", who, (long long)D0, (long long)D1, (long long)D2, kMaxExtent);
    PNP_REQUIRE(dims_ok(D0, D1, D2, n), "%s: %lld x %lld x %lld = %lld voxels, fewer than 2^31 are supported", who, (long long)D0, (long long)D1,
                (long long)D2, (long long)D0 * D1 * D2);
    PNP_REQUIRE(ncls >= 2 && ncls <= MAXC, "%s: ncls %d outside [2, %d]", who, (int)ncls, MAXC);
    return PNP_OK;
}

size_t ws_bytes_of(long long n) { return kHeaderBytes + (size_t)((4 * n + 255) / 256 * 256); }

// ---- hole filling -----------------------------------------------------------------------------------------------------------
// The background (label 0 or >= ncls) is labelled at connectivity 1 by the three launches above, as the one class of a 2-class volume
// `state`; a CAVITY is a background component without a voxel on a face of the volume.  A cavity's winner is the class with the most
// contacts (pairs of a cavity voxel and a face neighbour of class c; ties to the lower class); it is filled with its winner when
// class_mask holds the winner and max_size == 0 or size <= max_size.  After the labelling:
//   fh_open_kernel      one lane per FACE voxel: state[root] = kOpen, a plain store of a constant (racing stores write the same byte)
//   fh_prepare_kernel   roots only: sizes[root] = 0, and for closed roots the contact row = 0 (no clear of the whole table)
//   cc_count_kernel     sizes, merged in LDS: the open background of a scan costs one global add per workgroup
//   fh_contact_kernel   voxels of CLOSED components only: up to six neighbour labels, packed 4 bits per class, one global add per class met
//   fh_apply_kernel     every voxel of a cavity reads its root's row and size and decides alike; out may be vol (a lane reads and writes its
//                       own voxel only; the neighbours were read by the launch before); the root reports to the sums, merged in LDS
//   fh_stats_kernel     the int64 rows
// Each stage reads what an EARLIER launch wrote; integer atomics only, exact in any order.
constexpr unsigned char kBackground = 1, kOpen = 2;       // state: 0 = a class, 1 = background, 2 = background and the root of an open component

struct FillHeader {                        // the second kHeaderBytes of the fill workspace (the first are the Header above)
    unsigned int err_fill;                 // cavities without a contact, neighbours outside the volume (neither can happen)
    unsigned int pad;
    unsigned long long filled[MAXC], left[MAXC];          // per winner (cavities << 32) + voxels: filled / left as they are
    unsigned int largest[MAXC];            // the largest cavity filled with the class
};
static_assert(sizeof(FillHeader) <= kHeaderBytes, "fill header");

__global__ void __launch_bounds__(kThreads) fh_state_kernel(const unsigned char* __restrict__ vol, unsigned char* __restrict__ state, int n,
                                                            int ncls) {
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const unsigned char l = vol[v];
    state[v] = (l == 0 || l >= ncls) ? kBackground : 0;
}

__global__ void __launch_bounds__(kThreads) fh_open_kernel(const int* __restrict__ roots, unsigned char* state, int D0, int D1, int D2, int n) {
    int i = blockIdx.x * kThreads + threadIdx.x;          // < 2 (D1 D2 + D0 D2 + D0 D1) <= 6 * 2^24
    const int a0 = D1 * D2, a1 = D0 * D2, a2 = D0 * D1;
    int x, y, z;
    if (i < 2 * a0) {
        x = i < a0 ? 0 : D0 - 1;
        const int j = i < a0 ? i : i - a0;
        y = j / D2;
        z = j % D2;
    } else if ((i -= 2 * a0) < 2 * a1) {
        y = i < a1 ? 0 : D1 - 1;
        const int j = i < a1 ? i : i - a1;
        x = j / D2;
        z = j % D2;
    } else if ((i -= 2 * a1) < 2 * a2) {
        z = i < a2 ? 0 : D2 - 1;
        const int j = i < a2 ? i : i - a2;
        x = j / D1;
        y = j % D1;
    } else {
        return;
    }
    const int r = roots[(x * D1 + y) * D2 + z];
    if (r >= 0 && r < n) state[r] = kOpen;
}

__global__ void __launch_bounds__(kThreads) fh_prepare_kernel(const int* __restrict__ roots, const unsigned char* __restrict__ state,
                                                              int* __restrict__ sizes, int* __restrict__ contacts, int n, int nc1) {
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n || roots[v] != (int)v) return;
    sizes[v] = 0;
    if (state[v] == kOpen) return;
    for (int c = 0; c < nc1; ++c) contacts[(size_t)v * nc1 + c] = 0;
}

__global__ void __launch_bounds__(kThreads) fh_contact_kernel(const unsigned char* __restrict__ vol, const int* __restrict__ roots,
                                                              const unsigned char* __restrict__ state, int* contacts, FillHeader* fh,
                                                              int D0, int D1, int D2, int n, int ncls) {
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const int r = roots[v];
    if (r < 0 || r >= n || state[r] == kOpen) return;
    const int z = (int)(v % D2), t = (int)(v / D2), y = t % D1, x = t / D1;
    if (x < 1 || y < 1 || z < 1 || x > D0 - 2 || y > D1 - 2 || z > D2 - 2) {       // a closed component has no voxel on a face
        atomicAdd(&fh->err_fill, 1u);
        return;
    }
    const int sy = D2, sx = D1 * D2;
    const unsigned char nb[6] = {vol[v - sx], vol[v + sx], vol[v - sy], vol[v + sy], vol[v - 1], vol[v + 1]};
    unsigned int packed = 0;               // 4 bits per class: at most 6 contacts of a voxel
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (nb[j] >= 1 && nb[j] < ncls) packed += 1u << (4 * nb[j]);
    const int nc1 = ncls - 1;
    for (int c = 1; c < ncls; ++c) {
        const int k = (int)((packed >> (4 * c)) & 15u);
        if (k) atomicAdd(&contacts[(size_t)r * nc1 + c - 1], k);
    }
}

__global__ void __launch_bounds__(kThreads) fh_apply_kernel(const unsigned char* vol, const int* __restrict__ roots,
                                                            const unsigned char* __restrict__ state, const int* __restrict__ sizes,
                                                            const int* __restrict__ contacts, unsigned char* out, FillHeader* fh, int n, int ncls,
                                                            unsigned int mask, long long max_size) {
    __shared__ unsigned long long s_filled[MAXC], s_left[MAXC];
    __shared__ unsigned int s_largest[MAXC];
    if (threadIdx.x < MAXC) {
        s_filled[threadIdx.x] = s_left[threadIdx.x] = 0ull;
        s_largest[threadIdx.x] = 0u;
    }
    __syncthreads();
    const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (v < n) {
        unsigned char l = vol[v];
        if (l >= ncls) l = 0;
        const int r = roots[v];
        if (r >= 0 && r < n) {             // background
            l = 0;
            if (state[r] != kOpen) {       // a cavity
                const int nc1 = ncls - 1;
                int best = 0, win = 0;
                for (int c = 1; c < ncls; ++c) {
                    const int k = contacts[(size_t)r * nc1 + c - 1];
                    if (k > best) {        // ties stay with the lower class
                        best = k;
                        win = c;
                    }
                }
                const int s = sizes[r];
                const bool fill = win != 0 && ((mask >> win) & 1u) && (max_size == 0 || (long long)s <= max_size);
                if (fill) l = (unsigned char)win;
                if (r == (int)v) {         // the root reports its cavity
                    bad = win == 0;
                    const unsigned long long one = (1ull << 32) + (unsigned long long)(unsigned int)s;
                    if (fill) {
                        atomicAdd(&s_filled[win], one);
                        atomicMax(&s_largest[win], (unsigned int)s);
                    } else {
                        atomicAdd(&s_left[win], one);        // win == 0 (never): row 0 still counts it
                    }
                }
            }
        }
        out[v] = l;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < ncls) {
        if (s_filled[c] != 0ull) atomicAdd(&fh->filled[c], s_filled[c]);
        if (s_left[c] != 0ull) atomicAdd(&fh->left[c], s_left[c]);
        if (s_largest[c] != 0u) atomicMax(&fh->largest[c], s_largest[c]);
    }
    if (bad) atomicAdd(&fh->err_fill, 1u);
}

__global__ void fh_stats_kernel(const FillHeader* __restrict__ fh, long long* __restrict__ stats, int ncls) {
    const int c = threadIdx.x;
    if (c >= ncls) return;
    const unsigned long long lo = 0xffffffffull;
    if (c > 0) {
        stats[4 * c + 0] = (long long)(fh->filled[c] >> 32);
        stats[4 * c + 1] = (long long)(fh->filled[c] & lo);
        stats[4 * c + 2] = (long long)fh->largest[c];
        stats[4 * c + 3] = (long long)(fh->left[c] >> 32);
        return;
    }
    long long nf = 0, vf = 0, nl = 0, vl = 0;
    for (int k = 0; k < ncls; ++k) {
        nf += (long long)(fh->filled[k] >> 32);
        vf += (long long)(fh->filled[k] & lo);
        nl += (long long)(fh->left[k] >> 32);
        vl += (long long)(fh->left[k] & lo);
    }
    stats[0] = nf + nl;
    stats[1] = vf + vl;
    stats[2] = nl;
    stats[3] = vl;
}

// the fill workspace: Header, FillHeader, parent / sizes int32 [n], roots int32 [n], state uint8 [n], contacts int32 [n, ncls - 1];
// every block rounded up to 256 bytes
size_t round256(size_t b) { return (b + 255) / 256 * 256; }

size_t fill_ws_bytes_of(long long n, int ncls) {
    return 2 * kHeaderBytes + 2 * round256(4 * (size_t)n) + round256((size_t)n) + round256(4 * (size_t)n * (size_t)(ncls - 1));
}

}  // namespace

extern "C" {

size_t pnp_components_workspace_bytes(int64_t D0, int64_t D1, int64_t D2) {
    long long n;
    return dims_ok(D0, D1, D2, &n) ? ws_bytes_of(n) : 0;
}

int pnp_label_components(const uint8_t* vol, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, int32_t connectivity, int32_t* roots,
                         void* ws, size_t ws_bytes, void* stream) {
    PNP_REQUIRE(vol && roots && ws, "pnp_label_components: null pointer");
    long long n;
    if (const int rc = check_dims("pnp_label_components", D0, D1, D2, ncls, &n)) return rc;
    PNP_REQUIRE(connectivity >= 1 && connectivity <= 3, "pnp_label_components: connectivity %d outside {1, 2, 3}", (int)connectivity);
    PNP_REQUIRE(ws_bytes >= ws_bytes_of(n), "pnp_label_components: workspace too small (%zu < %zu bytes)", ws_bytes, ws_bytes_of(n));
    hipStream_t st = (hipStream_t)stream;
    Header* h = (Header*)ws;
    int* parent = (int*)((char*)ws + kHeaderBytes);
    Dims d;
    d.D0 = (int)D0; d.D1 = (int)D1; d.D2 = (int)D2;
    d.nt1 = pnp_cdiv(D1, T1);
    d.nt2 = pnp_cdiv(D2, T2);
    const unsigned tiles = (unsigned)((long long)pnp_cdiv(D0, T0) * d.nt1 * d.nt2);       // <= 512 * 512 * 128
    const int noff = connectivity == 1 ? 3 : connectivity == 2 ? 9 : 13;
    if (hipMemsetAsync(&h->err_label, 0, sizeof(unsigned int), st) != hipSuccess) {
        pnp_set_error("pnp_label_components: clearing the error counter failed");
        return PNP_ELAUNCH;
    }
    hipLaunchKernelGGL(cc_tile_kernel, dim3(tiles), dim3(kThreads), 0, st, vol, parent, h, d, (int)ncls, noff);
    PNP_CHECK_LAUNCH("cc_tile_kernel");
    hipLaunchKernelGGL(cc_border_kernel, dim3(tiles), dim3(kThreads), 0, st, vol, parent, h, d, (int)ncls, noff, (int)n);
    PNP_CHECK_LAUNCH("cc_border_kernel");
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)pnp_cdiv(n, kThreads)), dim3(kThreads), 0, st, parent, roots, h, (int)n);
    PNP_CHECK_LAUNCH("cc_flatten_kernel");
    return PNP_OK;
}

int pnp_filter_components(const uint8_t* vol, const int32_t* roots, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, uint32_t class_mask,
                          int32_t keep, int64_t min_size, uint8_t* out, int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
    PNP_REQUIRE(vol && roots && out && stats && ws, "pnp_filter_components: null pointer");
    long long n;
    if (const int rc = check_dims("pnp_filter_components", D0, D1, D2, ncls, &n)) return rc;
    PNP_REQUIRE(keep >= 0 && keep <= kMaxKeep, "pnp_filter_components: keep %d outside [0, %d]", (int)keep, kMaxKeep);
    PNP_REQUIRE(min_size >= 0, "pnp_filter_components: min_size %lld is negative", (long long)min_size);
    PNP_REQUIRE((class_mask & 1u) == 0 && (class_mask >> ncls) == 0, "pnp_filter_components: class_mask 0x%x selects class 0 or a class >= ncls = %d",
                (unsigned)class_mask, (int)ncls);
    PNP_REQUIRE(ws_bytes >= ws_bytes_of(n), "pnp_filter_components: workspace too small (%zu < %zu bytes)", ws_bytes, ws_bytes_of(n));
    hipStream_t st = (hipStream_t)stream;
    Header* h = (Header*)ws;
    int* sizes = (int*)((char*)ws + kHeaderBytes);
    // everything but the labelling's counter: the filter's counter, the keys, the sums and the sizes
    if (hipMemsetAsync(&h->err_filter, 0, ws_bytes_of(n) - sizeof(unsigned int), st) != hipSuccess) {
        pnp_set_error("pnp_filter_components: clearing the workspace failed");
        return PNP_ELAUNCH;
    }
    const unsigned flat = (unsigned)pnp_cdiv(n, kThreads);
    hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)pnp_cdiv(n, kThreads * kRun)), dim3(kThreads), 0, st, roots, sizes, h, (int)n);
    PNP_CHECK_LAUNCH("cc_count_kernel");
    for (int rank = 0; rank < (keep > 1 ? keep : 1); ++rank) {
        hipLaunchKernelGGL(cc_rank_kernel, dim3(flat), dim3(kThreads), 0, st, vol, roots, sizes, h, (int)n, (int)ncls, (unsigned int)class_mask, rank);
        PNP_CHECK_LAUNCH("cc_rank_kernel");
    }
    hipLaunchKernelGGL(cc_apply_kernel, dim3(flat), dim3(kThreads), 0, st, vol, roots, sizes, out, h, (int)n, (int)ncls, (unsigned int)class_mask,
                       (int)keep, (long long)min_size);
    PNP_CHECK_LAUNCH("cc_apply_kernel");
    hipLaunchKernelGGL(cc_stats_kernel, dim3(1), dim3(64), 0, st, h, (long long*)stats, (int)ncls);
    PNP_CHECK_LAUNCH("cc_stats_kernel");
    return PNP_OK;
}

size_t pnp_fill_holes_workspace_bytes(int64_t D0, int64_t D1, int64_t D2, int32_t ncls) {
    long long n;
    return dims_ok(D0, D1, D2, &n) && ncls >= 2 && ncls <= MAXC ? fill_ws_bytes_of(n, (int)ncls) : 0;
}

int pnp_fill_holes(const uint8_t* vol, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, uint32_t class_mask, int64_t max_size, uint8_t* out,
                   int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
    PNP_REQUIRE(vol && out && stats && ws, "pnp_fill_holes: null pointer");
    long long n;
    if (const int rc = check_dims("pnp_fill_holes", D0, D1, D2, ncls, &n)) return rc;
    PNP_REQUIRE((class_mask & 1u) == 0 && (class_mask >> ncls) == 0, "pnp_fill_holes: class_mask 0x%x selects class 0 or a class >= ncls = %d",
                (unsigned)class_mask, (int)ncls);
    PNP_REQUIRE(max_size >= 0, "pnp_fill_holes: max_size %lld is negative", (long long)max_size);
    // cc_count_kernel reads roots as int4 and FillHeader holds 64-bit atomics: every block starts at a multiple of 256 bytes from ws
    PNP_REQUIRE((uintptr_t)ws % 16 == 0, "pnp_fill_holes: ws must be 16-byte aligned");
    // fh_apply_kernel reads and writes a lane's own voxel only: out is vol itself or shares no byte with it
    const uintptr_t v0 = (uintptr_t)vol, v1 = v0 + (uintptr_t)n, o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n;
    PNP_REQUIRE(o0 == v0 || o1 <= v0 || v1 <= o0, "pnp_fill_holes: out overlaps vol");
    PNP_REQUIRE(ws_bytes >= fill_ws_bytes_of(n, (int)ncls), "pnp_fill_holes: workspace too small (%zu < %zu bytes)", ws_bytes,
                fill_ws_bytes_of(n, (int)ncls));
    hipStream_t st = (hipStream_t)stream;
    Header* h = (Header*)ws;
    FillHeader* fh = (FillHeader*)((char*)ws + kHeaderBytes);
    char* p = (char*)ws + 2 * kHeaderBytes;
    int* parent = (int*)p;                 // sizes once the roots stand
    int* roots = (int*)(p += round256(4 * (size_t)n));
    unsigned char* state = (unsigned char*)(p += round256(4 * (size_t)n));
    int* contacts = (int*)(p += round256((size_t)n));
    if (hipMemsetAsync(ws, 0, 2 * kHeaderBytes, st) != hipSuccess) {
        pnp_set_error("pnp_fill_holes: clearing the headers failed");
        return PNP_ELAUNCH;
    }
    Dims d;
    d.D0 = (int)D0; d.D1 = (int)D1; d.D2 = (int)D2;
    d.nt1 = pnp_cdiv(D1, T1);
    d.nt2 = pnp_cdiv(D2, T2);
    const unsigned tiles = (unsigned)((long long)pnp_cdiv(D0, T0) * d.nt1 * d.nt2);
    const unsigned flat = (unsigned)pnp_cdiv(n, kThreads);
    const long long faces = 2 * (D1 * D2 + D0 * D2 + D0 * D1);
    hipLaunchKernelGGL(fh_state_kernel, dim3(flat), dim3(kThreads), 0, st, vol, state, (int)n, (int)ncls);
    PNP_CHECK_LAUNCH("fh_state_kernel");
    // the background as the one class of a 2-class volume, 6 neighbours
    hipLaunchKernelGGL(cc_tile_kernel, dim3(tiles), dim3(kThreads), 0, st, state, parent, h, d, 2, 3);
    PNP_CHECK_LAUNCH("cc_tile_kernel");
    hipLaunchKernelGGL(cc_border_kernel, dim3(tiles), dim3(kThreads), 0, st, state, parent, h, d, 2, 3, (int)n);
    PNP_CHECK_LAUNCH("cc_border_kernel");
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(flat), dim3(kThreads), 0, st, parent, roots, h, (int)n);
    PNP_CHECK_LAUNCH("cc_flatten_kernel");
    hipLaunchKernelGGL(fh_open_kernel, dim3((unsigned)pnp_cdiv(faces, kThreads)), dim3(kThreads), 0, st, roots, state, (int)D0, (int)D1, (int)D2,
                       (int)n);
    PNP_CHECK_LAUNCH("fh_open_kernel");
    hipLaunchKernelGGL(fh_prepare_kernel, dim3(flat), dim3(kThreads), 0, st, roots, state, parent, contacts, (int)n, (int)ncls - 1);
    PNP_CHECK_LAUNCH("fh_prepare_kernel");
    hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)pnp_cdiv(n, kThreads * kRun)), dim3(kThreads), 0, st, roots, parent, h, (int)n);
    PNP_CHECK_LAUNCH("cc_count_kernel");
    hipLaunchKernelGGL(fh_contact_kernel, dim3(flat), dim3(kThreads), 0, st, vol, roots, state, contacts, fh, (int)D0, (int)D1, (int)D2, (int)n,
                       (int)ncls);
    PNP_CHECK_LAUNCH("fh_contact_kernel");
    hipLaunchKernelGGL(fh_apply_kernel, dim3(flat), dim3(kThreads), 0, st, vol, roots, state, parent, contacts, out, fh, (int)n, (int)ncls,
                       (unsigned int)class_mask, (long long)max_size);
    PNP_CHECK_LAUNCH("fh_apply_kernel");
    hipLaunchKernelGGL(fh_stats_kernel, dim3(1), dim3(64), 0, st, fh, (long long*)stats, (int)ncls);
    PNP_CHECK_LAUNCH("fh_stats_kernel");
    return PNP_OK;
}

}  // extern "C"
