// union_find.h -- the lock-free union-find by index that components.hip (radius components) and regions.hip (regions over a
// neighbour list) share: find with path halving, unite by hooking the larger root under the smaller.  Both files' claim that their
// labels do not depend on the order in which lanes run rests on the argument below.
//
// UNION-FIND BY INDEX.  parent[v] is the identity on entry.
//   - A hook is an agent-scope compare-and-swap parent[ra]: ra -> rb with rb < ra, on a ROOT ra (it succeeds only while parent[ra]
//     == ra).  Path halving lowers parent[v] of a NON-root v to its grandparent with an agent-scope atomic min.  Both store a
//     smaller index of the same component over a larger one, so parent[v] <= v always, parent[v] never grows, and a node that
//     has stopped being a root never becomes one again.
//   - find therefore walks strictly decreasing indices: at most n steps, whatever value it reads -- a stale read (the per-XCD L2s are
//     not coherent with each other; the loads are relaxed agent-scope atomic loads) is an older, larger ancestor of the same
//     component, and the walk from it ends at a node that was a root when it was read.
//   - unite(a, b): ra = find(a), rb = find(b); equal: done (they were joined when the later of the two was read).  Otherwise hook the
//     larger under the smaller.  A failed swap returns the value another lane stored there, an ancestor of ra below ra; the retry
//     starts from THAT value (not from a plain re-read), so max(ra, rb) strictly decreases from one try to the next: at most n
//     tries.  After a successful hook a and b have a common ancestor for good, since links are only ever replaced by links to
//     ancestors.
//   - A component's final root is its smallest member: a root is never hooked under a larger index, and when all unites are done
//     every united pair shares its root, hence a whole component does, and the smallest member can have no parent but itself.  The
//     roots are read in a launch of their own (k_components_flatten), where every hook is visible.
//   - No lane ever waits for a value another lane has yet to write: no flag, no lock, no barrier; every loop ends by its own
//     progress.  Each loop still carries a trip cap of n + 1 that the argument above rules out; reaching it sets *status, which the
//     host turns into an error.
// The results do not depend on the order of the hooks: the partition is the transitive closure of the united pairs, and the root is
// a function of the partition.
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

namespace {

__device__ __forceinline__ int uf_load(int32_t *parent, int v)
{
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v as far as this lane can see, with path halving; cap: the trip cap (n + 1)
__device__ __forceinline__ int uf_find(int32_t *parent, int v, int cap, int32_t *status)
{
    for (int t = 0; t < cap; ++t) {
        const int p = uf_load(parent, v);
        if (p == v)
            return v;
        const int gp = uf_load(parent, p);
        if (gp < p) // v is no root and never will be again: point it at its grandparent (smaller, same component)
            __hip_atomic_fetch_min(parent + v, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = gp; // <= p < v
    }
    *status = 1;
    return v;
}

// joins the components of a and b; returns the root both had when it was done
__device__ __forceinline__ int uf_unite(int32_t *parent, int a, int b, int cap, int32_t *status)
{
    int ra = uf_find(parent, a, cap, status), rb = uf_find(parent, b, cap, status);
    for (int t = 0; t < cap; ++t) {
        if (ra == rb)
            return ra;
        if (ra < rb) {
            const int x = ra;
            ra = rb;
            rb = x;
        }
        int seen = ra; // hook the larger root under the smaller one, if it still is a root
        if (__hip_atomic_compare_exchange_strong(parent + ra, &seen, rb, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return rb;
        ra = uf_find(parent, seen, cap, status); // from what the swap returned: an ancestor of ra below ra
        rb = uf_find(parent, rb, cap, status);
    }
    *status = 1;
    return rb;
}

} // namespace

} // namespace gwbp
