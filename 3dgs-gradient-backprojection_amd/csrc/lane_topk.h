// lane_topk.h -- a lane's private pair of LDS columns, [k][T] floats then [k][T] ints (one column per lane of a T-lane workgroup, so
// the lanes of a wave touch consecutive words), and the sorted top-k list that k_spatial_knn and k_point_gaussians keep in it.
// Columns are lane-private: no atomics, no barrier.
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

namespace {

// the dynamic LDS of a workgroup of T lanes with k entries each
inline size_t lane_columns_bytes(int k, int T) { return (size_t)k * T * (sizeof(float) + sizeof(int)); }

template <int T>
struct LaneColumns {
    float *f; // entry j of this lane: f[j * T], i[j * T]
    int *i;
    __device__ __forceinline__ LaneColumns(float *smem, int k, int tid) : f(smem + tid), i(reinterpret_cast<int *>(smem + k * T) + tid) {}
};

constexpr int kNoIndex = 0x7FFFFFFF; // an empty slot of a list: orders after every real index at an equal key

// The two orders of the keys: which of two keys comes first, and the key of an empty slot (the last of the order).  Equal keys go
// by index ascending in both.
struct NearestFirst { // d2 ascending
    static __device__ __forceinline__ float empty() { return __builtin_inff(); }
    static __device__ __forceinline__ bool first(float a, float b) { return a < b; }
};
struct HeaviestFirst { // weight descending (a kept weight is > 0, so an open list takes anything)
    static __device__ __forceinline__ float empty() { return 0.0f; }
    static __device__ __forceinline__ bool first(float a, float b) { return a > b; }
};

// The k first entries, in Order, of everything offered.  The list's last entry -- the k-th best so far -- is cached in registers,
// so an offer that does not make the list costs no LDS access.
template <class Order, int T>
struct LaneTopK {
    LaneColumns<T> col;
    int k;
    float last_key;
    int last_id;

    __device__ __forceinline__ LaneTopK(float *smem, int k_, int tid) : col(smem, k_, tid), k(k_) {}
    __device__ __forceinline__ void init()
    {
        for (int j = 0; j < k; ++j) {
            col.f[j * T] = Order::empty();
            col.i[j * T] = kNoIndex;
        }
        last_key = Order::empty();
        last_id = kNoIndex;
    }
    __device__ __forceinline__ void offer(float key, int id)
    {
        if (Order::first(key, last_key) || (key == last_key && id < last_id)) {
            int j = k - 1; // sorted insert: shift the entries that order after (key, id) one down
            while (j > 0) {
                const float pk = col.f[(j - 1) * T];
                const int pi = col.i[(j - 1) * T];
                if (Order::first(pk, key) || (pk == key && pi < id))
                    break;
                col.f[j * T] = pk;
                col.i[j * T] = pi;
                --j;
            }
            col.f[j * T] = key;
            col.i[j * T] = id;
            last_key = col.f[(k - 1) * T];
            last_id = col.i[(k - 1) * T];
        }
    }
    // entry j as it is written back: the key (Order::empty() in an empty slot), and the index with -1 for an empty slot
    __device__ __forceinline__ float key(int j) const { return col.f[j * T]; }
    __device__ __forceinline__ int index(int j) const
    {
        const int id = col.i[j * T];
        return id == kNoIndex ? -1 : id;
    }
};

} // namespace

} // namespace gwbp
