// trie_build.h -- host entry points of the GPU trie hasher (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "arena.h"
#include "witness.h"

namespace phant {

// The sorted pairs of a forest of independent tries, DEVICE view: key_off / val_off relative to keys / vals (n + 1 entries each), the
// byte totals given by whoever packed them; trie t owns pairs [seg_first[t], seg_first[t + 1]); roots = n_tries x 32 bytes, written.
struct TriePairs {
    const uint8_t* keys = nullptr;
    const uint32_t* key_off = nullptr;
    uint64_t key_bytes = 0;
    const uint8_t* vals = nullptr;
    const uint64_t* val_off = nullptr;
    uint64_t val_bytes = 0;
    uint32_t n = 0;
    const uint32_t* seg_first = nullptr;  // n_tries + 1
    uint32_t n_tries = 1;
    uint8_t* roots = nullptr;
};
// ... and every trie's root NODE where it is wanted: RLP, cap bytes each; len 0 for an empty trie, possibly > cap -- then the bytes
// were not written
struct RootNodes {
    uint8_t* enc = nullptr;
    uint32_t* len = nullptr;
    uint32_t cap = 0;
};
// The same pairs, HOST view: the offsets may begin anywhere (staging.h: stage_pairs rebases them); key_off / val_off may be null
// with n == 0, seg_first with n_tries == 1 (one trie over all pairs).
struct HostPairs {
    const uint8_t* keys = nullptr;
    const uint32_t* key_off = nullptr;
    const uint8_t* vals = nullptr;
    const uint64_t* val_off = nullptr;
    uint32_t n = 0;
    const uint32_t* seg_first = nullptr;
    uint32_t n_tries = 1;
};
// the keys a prover is asked about, in either view
struct ProveQueries {
    const uint8_t* qkeys = nullptr;
    const uint32_t* qkey_off = nullptr;  // n_queries + 1 (may be null with n_queries == 0 in the host view)
    const uint32_t* q_trie = nullptr;    // optional: the trie of query j (else trie 0)
    const uint8_t* q_flags = nullptr;    // optional: PHANT_PROVE_*
    uint32_t n_queries = 0;
};

// mptize (src/mpt/mpt.zig:38-45) over a forest in host memory: H2D, build + hash on the GPU, roots_out = n_tries x 32 bytes (and the
// root nodes, to host buffers) back.  Returns PHANT_OK / PHANT_E_*; err gets a message.
int32_t trie_forest_host(Workspaces& ws, hipStream_t st, const HostPairs& h, uint8_t* roots_out, std::string& err, const RootNodes& nodes_out = {});

// mptize of ONE trie over device-resident arrays (p.seg_first ignored); the root lands in p.roots (device).  The pass reads two small
// counter blocks back in between (depth bins, the UNSORTED flag), i.e. it synchronises the stream twice.
int32_t trie_root_dev(Workspaces& ws, hipStream_t st, const TriePairs& p, std::string& err);

// the forest pass over device-resident arrays (segment table and roots in device memory too); t1 / t2 arenas only
int32_t trie_forest_dev(Workspaces& ws, hipStream_t st, const TriePairs& p, std::string& err);

// ... and with every trie's root NODE; these small results are delivered to HOST buffers (the call synchronises); d_out:
// n_tries x (36 + out.cap) + 64 bytes of device memory (4-byte aligned) they pass through (p.roots ignored)
int32_t trie_forest_nodes_dev(Workspaces& ws, hipStream_t st, const TriePairs& p, uint8_t* d_out, uint8_t* roots_out, const RootNodes& out,
                              std::string& err);

// Witness generation (kernels in trie_prove.hip.h; the host driver's stages: DESIGN.md section 7d): the forest pass with its tables
// kept, then the hashed nodes on the paths of the queried keys -- as one node set, every node once (phant_mpt_prove_nodeset), or
// with per_proof as every query's own ordered node list, root first, the lists back to back in query order (phant_mpt_prove_batch;
// q.q_flags is not read).  The queries and the caller's output buffers (any may be null: not wanted); total_nodes / nodes_len are
// always written, node bytes and offsets only when both fit their capacities.  first_node is the set's trie_first_node (n_tries + 1,
// written whether or not the rest fits) or the proofs' proof_first_node (n_queries + 1, written with the rest).
struct ProveArgs {
    ProveQueries q;
    bool per_proof = false;
    uint8_t* nodes = nullptr;
    uint64_t nodes_cap = 0;
    uint64_t* node_off = nullptr;    // max_nodes + 1
    uint32_t max_nodes = 0;
    uint32_t* first_node = nullptr;  // n_tries + 1 | n_queries + 1
    uint8_t* roots = nullptr;        // n_tries x 32
    uint8_t* q_status = nullptr;     // n_queries
    uint32_t total_nodes = 0;        // out
    uint64_t nodes_len = 0;          // out
};
// every array in host memory
int32_t prove_host(Workspaces& ws, hipStream_t st, const HostPairs& h, ProveArgs& a, std::string& err);
// every array of `a` and of the forest in device memory (p.seg_first null with n_tries == 1: one trie; p.roots ignored: a.roots)
int32_t prove_dev(Workspaces& ws, hipStream_t st, const TriePairs& p, ProveArgs& a, std::string& err);

// the proving forest pass of a caller that owns ws.io (everything device-resident, p.seg_first / p.roots required): the set's nodes
// are appended to the host vectors (node_off: one entry per node so far + 1); with `first` the per-proof form, whose proofs REPLACE
// the vectors' contents (node_off: total_nodes + 1 entries, first: n_queries + 1)
int32_t prove_collect(Workspaces& ws, hipStream_t st, const TriePairs& p, const ProveQueries& q, std::vector<uint8_t>& nodes,
                      std::vector<uint64_t>& node_off, std::vector<uint32_t>* first, std::string& err);

// calculateMPTRoot (src/blockchain/blockchain.zig:209-235) when !be32,
// ExecutionPayload.toBlock keys (src/engine_api/execution_payload.zig:127-139)
// when be32.
int32_t index_root_host(Workspaces& ws, hipStream_t st, const uint8_t* items, const uint64_t* item_off, uint32_t n,
                        bool be32, uint8_t out[32], std::string& err);

// calculateMPTRoot of n_lists lists in one forest pass (blockchain.zig:198-204); roots_out = n_lists x 32 bytes
int32_t index_roots_host(Workspaces& ws, hipStream_t st, const uint8_t* const* items, const uint64_t* const* item_off,
                         const uint32_t* n, uint32_t n_lists, uint8_t* roots_out, std::string& err);

// The AccountState fields (src/state/types.zig:13-20) as struct-of-arrays, in host or in device memory.  Host view: the offsets may
// begin anywhere, m / code_bytes are not read.  Device view: offsets relative (code_off[0] == 0, slot_first[0] == 0), m and code_bytes
// given by whoever packed the arrays.
struct StateIn {
    const uint8_t* addrs = nullptr;        // n x 20
    const uint64_t* nonces = nullptr;      // n
    const uint8_t* bal = nullptr;          // n x 32, big-endian
    const uint8_t* code = nullptr;         // code_bytes
    const uint64_t* code_off = nullptr;    // n + 1
    const uint8_t* skeys = nullptr;        // m x 32
    const uint8_t* svals = nullptr;        // m x 32 (4-byte aligned)
    const uint32_t* slot_first = nullptr;  // n + 1
    uint32_t n = 0, m = 0;
    uint64_t code_bytes = 0;
};

// secure-trie state root over a state in host memory
int32_t state_root_host(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t out[32], std::string& err);

// phant_state_witness: the same pass with the touched keys (host view; 20-byte address | 52-byte address ++ slot; q_flags may be
// null, q_trie is not read) proven against both forests: `w` as the parser would return it for the document, root_out the state root
int32_t state_witness_host(Workspaces& ws, hipStream_t st, const StateIn& in, const ProveQueries& touched, ExecWitness& w, uint8_t root_out[32],
                           std::string& err);

// phant_state_proofs: the same pass with the keys (host view, as above; q_flags / q_trie are not read) proven in the per-proof
// form: `w` as witness_parse_json would return it for the EIP-1186 document, root_out the state root
int32_t state_proofs_host(Workspaces& ws, hipStream_t st, const StateIn& in, const ProveQueries& keys, Witness& w, uint8_t root_out[32],
                          std::string& err);

// the same over a DEVICE-resident state, the root written to device memory
int32_t state_root_dev(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t* d_root, std::string& err);

// one device's share of a sharded state root: its accounts' sub-tries by the top nibble of the hashed address -- roots
// (16 x 32), root nodes (16 x cap) and their lengths (0: no account there); the leaves stay on the device
int32_t state_subtrie_nodes_host(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t* roots, const RootNodes& out, std::string& err);

// the sorted leaves of that trie (keys n x 32 = keccak256(address) ascending, values = account RLP, val_off
// n + 1), storage roots included: what a rank of a sharded state root feeds to the top-nibble exchange
int32_t state_leaves_host(Workspaces& ws, hipStream_t st, const StateIn& in, std::vector<uint8_t>& keys, std::vector<uint8_t>& vals,
                          std::vector<uint64_t>& val_off, std::string& err);

}  // namespace phant
