// fs_median_sort.h — the goal point of a frontier piece (FrontierSearch.cpp:158-170 / 193-205, FRONTIER_POINT_MEDIAN): the piece's
// cells sorted by SortByMedianFunctor (FrontierSearch.hpp:156-181) with libstdc++'s std::sort, then the middle element.
//
// The comparator is not a strict weak order (a first-quadrant angle never sorts before a fourth-quadrant one, so three angle
// ranges form a cycle), and the element std::sort leaves in the middle depends on its exact sequence of comparisons and moves.
// This header restates that sequence (libstdc++'s std::__sort: introsort with _S_threshold = 16, median of three moved to the
// first position, unguarded partition, heap-sort fallback at depth 2 * floor(log2 n), final insertion sort) so that the device
// and a host test compile the same source.  The recursion of __introsort_loop becomes an explicit stack processed in the same
// order (right part first, then the left part), so a cyclic input touches the array in the same sequence.
//
// One deliberate difference: libstdc++'s unguarded scans can walk past either end of the WHOLE array on a cyclic input (undefined
// behaviour in the reference).  Here every unguarded scan stops at the array's ends; fs_msort_sort returns how many times a scan
// was stopped, so a caller can tell an exact restatement (0) from a guarded one.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_MSORT_HD __host__ __device__
#else
#define FS_MSORT_HD
#endif

#define FS_MSORT_PI 3.14159265358979323846      // M_PI

// one cell of a piece: its angle about the piece's centroid, and who it is
struct fs_msort_elem {
    double angle;
    int32_t cell;
};

// SortByMedianFunctor's angle: atan2 about the centroid, folded into [0, 2 pi)
FS_MSORT_HD inline double fs_msort_angle(double dy, double dx)
{
    double a = atan2(dy, dx);
    if (a < 0) a = a + (2 * FS_MSORT_PI);
    return a;
}

// SortByMedianFunctor::operator() on two angles
FS_MSORT_HD inline bool fs_msort_less(double aa, double ab)
{
    if (0 <= aa && aa <= FS_MSORT_PI / 2 && 3 * FS_MSORT_PI / 2 <= ab && ab <= 2 * FS_MSORT_PI) return false;
    if (0 <= ab && ab <= FS_MSORT_PI / 2 && 3 * FS_MSORT_PI / 2 <= aa && aa <= 2 * FS_MSORT_PI) return true;
    return aa < ab;
}

// the generic restatement: T any copyable element, Less(const T &, const T &) -> bool.  Indices are relative to `a`, whose n
// elements are the whole array (the guards' bounds).
template <class T, class Less>
struct fs_msort {
    T *a;
    int64_t n;
    Less less;
    int32_t guarded;

    FS_MSORT_HD void swap(int64_t i, int64_t j) { const T t = a[i]; a[i] = a[j]; a[j] = t; }

    // std::__move_median_to_first
    FS_MSORT_HD void median_to_first(int64_t r, int64_t x, int64_t y, int64_t z)
    {
        if (less(a[x], a[y])) {
            if (less(a[y], a[z])) swap(r, y);
            else if (less(a[x], a[z])) swap(r, z);
            else swap(r, x);
        } else if (less(a[x], a[z])) swap(r, x);
        else if (less(a[y], a[z])) swap(r, z);
        else swap(r, y);
    }

    // std::__unguarded_partition(first, last, pivot)
    FS_MSORT_HD int64_t partition(int64_t first, int64_t last, int64_t pivot)
    {
        for (;;) {
            while (less(a[first], a[pivot])) {
                if (first + 1 >= n) { ++guarded; break; }
                ++first;
            }
            --last;
            while (less(a[pivot], a[last])) {
                if (last == 0) { ++guarded; break; }
                --last;
            }
            if (!(first < last)) return first;
            swap(first, last);
            ++first;
        }
    }

    // std::__adjust_heap + std::__push_heap over a[first, first + len)
    FS_MSORT_HD void adjust_heap(int64_t first, int64_t hole, int64_t len, T value)
    {
        const int64_t top = hole;
        int64_t second = hole;
        while (second < (len - 1) / 2) {
            second = 2 * (second + 1);
            if (less(a[first + second], a[first + (second - 1)])) second--;
            a[first + hole] = a[first + second];
            hole = second;
        }
        if ((len & 1) == 0 && second == (len - 2) / 2) {
            second = 2 * (second + 1);
            a[first + hole] = a[first + (second - 1)];
            hole = second - 1;
        }
        int64_t parent = (hole - 1) / 2;
        while (hole > top && less(a[first + parent], value)) {
            a[first + hole] = a[first + parent];
            hole = parent;
            parent = (hole - 1) / 2;
        }
        a[first + hole] = value;
    }

    // std::__partial_sort(first, last, last): __heap_select (only __make_heap when middle == last) + __sort_heap
    FS_MSORT_HD void heap_sort(int64_t first, int64_t last)
    {
        const int64_t len = last - first;
        if (len >= 2) {
            for (int64_t parent = (len - 2) / 2;; --parent) {
                adjust_heap(first, parent, len, a[first + parent]);
                if (parent == 0) break;
            }
        }
        while (last - first > 1) {                   // __sort_heap: __pop_heap(first, last - 1, last - 1)
            --last;
            const T value = a[last];
            a[last] = a[first];
            adjust_heap(first, 0, last - first, value);
        }
    }

    // std::__unguarded_linear_insert(last)
    FS_MSORT_HD void linear_insert(int64_t last)
    {
        const T val = a[last];
        int64_t next = last - 1;
        while (less(val, a[next])) {
            a[last] = a[next];
            last = next;
            if (next == 0) { ++guarded; break; }
            --next;
        }
        a[last] = val;
    }

    // std::__insertion_sort
    FS_MSORT_HD void insertion_sort(int64_t first, int64_t last)
    {
        if (first == last) return;
        for (int64_t i = first + 1; i != last; ++i) {
            if (less(a[i], a[first])) {
                const T val = a[i];
                for (int64_t k = i; k > first; --k) a[k] = a[k - 1];
                a[first] = val;
            } else {
                linear_insert(i);
            }
        }
    }

    // std::__sort(a, a + n)
    FS_MSORT_HD void sort()
    {
        if (n <= 1) return;
        int lg = 0;
        for (int64_t m = n; m > 1; m >>= 1) ++lg;    // std::__lg
        // __introsort_loop: a frame is (first, last, depth); the recursion on [cut, last) runs before the loop goes on with
        // [first, cut), so [first, cut) is pushed and [cut, last) continued.  At most 2 lg + 1 frames are pending (n < 2^31).
        int64_t st_first[64], st_last[64];
        int st_depth[64];
        int top = 0;
        int64_t first = 0, last = n;
        int depth = 2 * lg;
        for (;;) {
            if (last - first > 16) {
                if (depth == 0) {
                    heap_sort(first, last);
                } else {
                    --depth;
                    const int64_t mid = first + (last - first) / 2;
                    median_to_first(first, first + 1, mid, last - 1);
                    const int64_t cut = partition(first + 1, last, first);
                    st_first[top] = first; st_last[top] = cut; st_depth[top] = depth; ++top;
                    first = cut;
                    continue;
                }
            }
            if (top == 0) break;
            --top;
            first = st_first[top]; last = st_last[top]; depth = st_depth[top];
        }
        // __final_insertion_sort
        if (n > 16) {
            insertion_sort(0, 16);
            for (int64_t i = 16; i != n; ++i) linear_insert(i);
        } else {
            insertion_sort(0, n);
        }
    }
};

struct fs_msort_elem_less {
    FS_MSORT_HD bool operator()(const fs_msort_elem &u, const fs_msort_elem &v) const { return fs_msort_less(u.angle, v.angle); }
};

// sorts a[0, n) as the reference's std::sort with SortByMedianFunctor would; returns the number of guarded scan stops
FS_MSORT_HD inline int32_t fs_msort_sort(fs_msort_elem *a, int64_t n)
{
    fs_msort<fs_msort_elem, fs_msort_elem_less> s{a, n, fs_msort_elem_less{}, 0};
    s.sort();
    return s.guarded;
}
