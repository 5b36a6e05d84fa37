// dbg_hash_check.cpp — TEST-ONLY host build of the product's dbg hash and table sizing (genomicsbench_amd/csrc/dbg_hash.h,
// the header dbg_kernels.hip includes), so that tests/dbg_cases.py's restatement of them, and with it the frozen colliding
// k-mers, are held against what the kernel computes.  g++ -O2 -std=c++17 -fPIC -shared (tests/test_dbg_edges_cpu.py).
#include "../../genomicsbench_amd/csrc/dbg_hash.h"

extern "C" {

void hostcheck_dbg_node(const uint8_t *bytes, int k, int64_t nc, uint64_t *tag, uint64_t *home)
{
    const uint64_t h = gbx::dbg_mix64(gbx::dbg_fnv(bytes, k));
    *tag = gbx::dbg_node_tag(h);
    *home = gbx::dbg_node_home(h, nc);
}

void hostcheck_dbg_edge(int64_t slot, int byte, int64_t ec, uint64_t *home)
{
    *home = gbx::dbg_edge_home(gbx::dbg_edge_key(slot, (uint8_t)byte), ec);
}

void hostcheck_dbg_sizes(int64_t C, int64_t *nc, int64_t *ec)
{
    *nc = gbx::dbg_node_slots(C);
    *ec = gbx::dbg_edge_slots(C);
}

// many k-mers at once (n rows of k bytes): the CPU test's bulk comparison
void hostcheck_dbg_nodes(const uint8_t *bytes, int64_t n, int k, int64_t nc, uint64_t *tag, uint64_t *home)
{
    for (int64_t i = 0; i < n; ++i) hostcheck_dbg_node(bytes + i * k, k, nc, tag + i, home + i);
}

}  // extern "C"
