// Test aid of tests/pc_restatement.py: libstdc++ std::unordered_set<int> built and filled the ways learning/algorithms/pc.cpp and
// constraint.hpp do it - the range constructor sizes its bucket array from the range, so the iteration order of such a set differs from
// that of one filled element by element.
#include <unordered_set>

using Set = std::unordered_set<int>;

extern "C" {
void* uset_new(void) { return new Set(); }
void* uset_from_range(const int* v, int n) { return new Set(v, v + n); }
void uset_free(void* h) { delete (Set*)h; }
void uset_insert(void* h, int v) { ((Set*)h)->insert(v); }
void uset_insert_range(void* h, const int* v, int n) { ((Set*)h)->insert(v, v + n); }
void uset_erase(void* h, int v) { ((Set*)h)->erase(v); }
int uset_count(void* h, int v) { return (int)((Set*)h)->count(v); }
int uset_size(void* h) { return (int)((Set*)h)->size(); }
void uset_items(void* h, int* out) {
    int i = 0;
    for (int v : *(Set*)h) out[i++] = v;
}
}
