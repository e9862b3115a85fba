// host_rlp.h -- host-only RLP helpers of the C-ABI (no HIP anywhere): the consistency check of
// phant_witness_verify and phant_mpt_strip_first_nibble.  Kept apart from capi.hip so that they can be
// built with plain g++ under sanitizers (tests/native/).
#pragma once
#include <cstddef>
#include <cstdint>

#include <vector>

#include "witness.h"

namespace phant {

// one canonical RLP item of `avail` bytes at p: payload offset / length, or false
bool host_rlp_item(const uint8_t* p, size_t avail, size_t& pay, size_t& len, size_t& total, bool& is_list);
// big-endian minimal integer string == the 32-byte padded declaration?
bool be_equals_padded(const uint8_t* v, size_t len, const uint8_t padded[32]);
// Does the proven account leaf rlp([nonce, balance, storageRoot, codeHash]) agree with the declaration?
bool account_consistent(const WitnessAccount& a, const uint8_t* value, size_t vlen);
// An account proven ABSENT: the declaration must describe the empty account
bool account_absent_consistent(const WitnessAccount& a);
// phant_mpt_strip_first_nibble (include/phant_gpu.h): returns PHANT_OK / PHANT_E_*
int32_t strip_first_nibble(const uint8_t* node, uint32_t len, uint8_t* out, uint32_t cap, uint32_t* out_len,
                           uint32_t* is_ref);

// phant_tx_senders (include/phant_gpu.h): one raw transaction -> PHANT_SIG_OK with its signing preimage APPENDED to `preimage`,
// r and s padded to 32 bytes and the recovery id, or PHANT_SIG_BAD_TX / PHANT_SIG_BAD_V (nothing appended).  Untrusted bytes in.
uint8_t tx_signing_parts(const uint8_t* tx, size_t len, uint64_t chain_id, std::vector<uint8_t>& preimage, uint8_t r[32],
                         uint8_t s[32], uint8_t* recid);

// phant_headers_decode_rlp (include/phant_gpu.h): header i of the call, strictly decoded from `len` bytes at `p` (from_block: the
// first item of the block encoding there) into row i of the caller's arrays behind `f`; extra_data is appended at *extra_at.
// false = refused: row i is zeroed, its n_fields is 0 and *extra_at stays.  Untrusted bytes in.
struct HeaderArrays {
    uint8_t *parent_hash, *uncle_hash, *fee_recipient, *state_root, *transactions_root, *receipts_root, *logs_bloom;
    uint64_t *difficulty, *number, *gas_limit, *gas_used, *timestamp;
    uint8_t* extra_data;
    uint32_t* extra_off;
    uint8_t *prev_randao, *nonce, *base_fee, *withdrawals_root;
    uint64_t *blob_gas_used, *excess_blob_gas;
    uint8_t *parent_beacon_root, *requests_hash, *n_fields;
};
bool header_decode(const uint8_t* p, size_t len, bool from_block, const HeaderArrays& f, uint32_t i, uint32_t* extra_at);

// phant_bodies_decode_rlp (include/phant_gpu.h): one raw block (has_header) or body of `len` bytes at `p` -> PHANT_SPLIT_*.  On
// PHANT_SPLIT_OK its transactions and withdrawals are counted into `t`, and with a sink their values are first appended at t's
// positions (tx_off[t.n + 1 ..], wd_off[t.n_wd + 1 ..]: the caller has made room and set entry 0); a refused block changes nothing.
// Untrusted bytes in.
struct BodyTotals {
    uint64_t n, n_wd, tx_bytes, wd_bytes;
};
struct BodySink {
    uint8_t* txs;
    uint64_t* tx_off;
    uint8_t* wd;
    uint64_t* wd_off;
};
uint8_t body_split(const uint8_t* p, size_t len, bool has_header, BodyTotals& t, const BodySink* sink);

// phant_receipts_decode_rlp (include/phant_gpu.h): the receipts list of one block, `len` bytes at `p` -> PHANT_SPLIT_OK,
// PHANT_SPLIT_BAD_RLP or PHANT_SPLIT_BAD_RECEIPT.  On PHANT_SPLIT_OK its values are counted into `t`, and with a sink first appended
// at t's positions (rc_off[t.n + 1 ..]); a refused block changes nothing.  The receipts are not looked into.  Untrusted bytes in.
struct ReceiptTotals {
    uint64_t n, bytes;
};
struct ReceiptSink {
    uint8_t* receipts;
    uint64_t* rc_off;
};
uint8_t receipts_split(const uint8_t* p, size_t len, bool eth69, ReceiptTotals& t, const ReceiptSink* sink);

}  // namespace phant
