// host_rlp.cpp -- see host_rlp.h.  Pure host code: untrusted bytes in, no HIP call.
#include "host_rlp.h"

#include <cstring>
#include <vector>

#include "../../include/phant_gpu.h"
#include "rlp.h"

namespace phant {


// one canonical RLP item of `avail` bytes at p: payload offset / length, or false (rlp.h's decoder over size_t offsets)
bool host_rlp_item(const uint8_t* p, size_t avail, size_t& pay, size_t& len, size_t& total, bool& is_list) {
    RlpItemOf<size_t> it;
    if (!rlp_decode(MemBytes{p}, 0, avail, it)) return false;
    pay = it.pay, len = it.len, total = it.total, is_list = it.is_list != 0;
    return true;
}

// big-endian minimal integer string == the 32-byte padded declaration?
bool be_equals_padded(const uint8_t* v, size_t len, const uint8_t padded[32]) {
    if (len > 32 || (len && v[0] == 0)) return false;
    for (size_t i = 0; i < 32 - len; ++i)
        if (padded[i]) return false;
    return std::memcmp(padded + 32 - len, v, len) == 0;
}

static const uint8_t EMPTY_ROOT[32] = {0x56, 0xe8, 0x1f, 0x17, 0x1b, 0xcc, 0x55, 0xa6, 0xff, 0x83, 0x45, 0xe6, 0x92, 0xc0, 0xf8, 0x6e,
                                0x5b, 0x48, 0xe0, 0x1b, 0x99, 0x6c, 0xad, 0xc0, 0x01, 0x62, 0x2f, 0xb5, 0xe3, 0x63, 0xb4, 0x21};
static const uint8_t EMPTY_CODE[32] = {0xc5, 0xd2, 0x46, 0x01, 0x86, 0xf7, 0x23, 0x3c, 0x92, 0x7e, 0x7d, 0xb2, 0xdc, 0xc7, 0x03, 0xc0,
                                0xe5, 0x00, 0xb6, 0x53, 0xca, 0x82, 0x27, 0x3b, 0x7b, 0xfa, 0xd8, 0x04, 0x5d, 0x85, 0xa4, 0x70};

// Does the proven account leaf agree with the declaration?  value = rlp([nonce, balance, storageRoot, codeHash])
bool account_consistent(const WitnessAccount& a, const uint8_t* value, size_t vlen) {
    size_t pay, len, total;
    bool is_list;
    if (!host_rlp_item(value, vlen, pay, len, total, is_list) || !is_list || total != vlen) return false;
    const uint8_t* p = value + pay;
    size_t left = len;
    const uint8_t* item[4];
    size_t ilen[4];
    for (int k = 0; k < 4; ++k) {
        size_t ip, il, it;
        bool il_list;
        if (!host_rlp_item(p, left, ip, il, it, il_list) || il_list) return false;
        item[k] = p + ip;
        ilen[k] = il;
        p += it;
        left -= it;
    }
    if (left) return false;
    if (ilen[2] != 32 || std::memcmp(item[2], a.storage_hash, 32) != 0) return false;
    if (a.has_code_hash && (ilen[3] != 32 || std::memcmp(item[3], a.code_hash, 32) != 0)) return false;
    if (a.has_balance && !be_equals_padded(item[1], ilen[1], a.balance)) return false;
    if (a.has_nonce) {
        uint8_t n32[32] = {0};
        for (int i = 0; i < 8; ++i) n32[31 - i] = (uint8_t)(a.nonce >> (8 * i));
        if (!be_equals_padded(item[0], ilen[0], n32)) return false;
    }
    return true;
}

bool account_absent_consistent(const WitnessAccount& a) {
    static const uint8_t zero[32] = {0};
    if (std::memcmp(a.storage_hash, EMPTY_ROOT, 32) != 0) return false;
    if (a.has_code_hash && std::memcmp(a.code_hash, EMPTY_CODE, 32) != 0) return false;
    if (a.has_balance && std::memcmp(a.balance, zero, 32) != 0) return false;
    if (a.has_nonce && a.nonce != 0) return false;
    return true;
}

int32_t strip_first_nibble(const uint8_t* node, uint32_t len, uint8_t* out, uint32_t cap, uint32_t* out_len,
                                     uint32_t* is_ref) {
    if (!node || !out || !out_len || !is_ref) return PHANT_E_INVALID_ARG;
    size_t pay, plen, total, ip, il, it;
    bool is_list, item_list;
    if (!host_rlp_item(node, len, pay, plen, total, is_list) || !is_list || total != len) return PHANT_E_INVALID_ARG;
    const uint8_t* p = node + pay;
    // item 0: the hex-prefix path (mpt.zig:285-314)
    if (!host_rlp_item(p, plen, ip, il, it, item_list) || item_list || il == 0) return PHANT_E_INVALID_ARG;
    const uint8_t* hp = p + ip;
    const uint32_t flag = hp[0] >> 4;
    if (flag > 3) return PHANT_E_INVALID_ARG;
    const bool leaf = flag & 2u, odd = flag & 1u;
    // item 1: value (leaf) or child reference (extension), kept as it is
    const uint8_t* rest = p + it;
    const size_t rest_len = plen - it;
    size_t rp, rl, rt;
    bool rlist;
    if (!host_rlp_item(rest, rest_len, rp, rl, rt, rlist) || rt != rest_len) return PHANT_E_INVALID_ARG;  // 2 items
    std::vector<uint8_t> nib;
    if (odd) nib.push_back(hp[0] & 0x0f);
    else if (hp[0] & 0x0f) return PHANT_E_INVALID_ARG;
    for (size_t k = 1; k < il; ++k) {
        nib.push_back(hp[k] >> 4);
        nib.push_back(hp[k] & 0x0f);
    }
    if (nib.empty()) return PHANT_E_INVALID_ARG;  // nothing to strip
    nib.erase(nib.begin());
    if (nib.empty() && !leaf) {
        // the extension only carried that one nibble: one level lower sits its child, as the reference says
        *is_ref = 1;
        if (!rlist && rl == 32) {
            if (cap < 32) return PHANT_E_INVALID_ARG;
            std::memcpy(out, rest + rp, 32);
            *out_len = 32;
        } else if (rlist && rt < 32) {
            if (cap < rt) return PHANT_E_INVALID_ARG;
            std::memcpy(out, rest, rt);
            *out_len = (uint32_t)rt;
        } else {
            return PHANT_E_INVALID_ARG;
        }
        return PHANT_OK;
    }
    // re-encode [HP(nib), item1]
    std::vector<uint8_t> h;
    const uint8_t f = (uint8_t)((leaf ? 2 : 0) | (nib.size() & 1));
    size_t k = 0;
    if (nib.size() & 1) h.push_back((uint8_t)(f << 4 | nib[k++]));
    else h.push_back((uint8_t)(f << 4));
    for (; k + 1 < nib.size(); k += 2) h.push_back((uint8_t)(nib[k] << 4 | nib[k + 1]));
    uint8_t hdr[9];
    std::vector<uint8_t> body(str_len(h.size(), h[0]));  // (keys go up to 255 bytes, 128 path bytes: beyond the short form)
    (void)put_str(body.data(), h.data(), (uint32_t)h.size());
    body.insert(body.end(), rest, rest + rest_len);
    std::vector<uint8_t> enc(hdr, hdr + put_hdr(hdr, 0xc0u, body.size()));
    enc.insert(enc.end(), body.begin(), body.end());
    *is_ref = 0;
    *out_len = (uint32_t)enc.size();
    if (enc.size() > cap) return PHANT_E_OOM;  // out_len says how much is needed
    std::memcpy(out, enc.data(), enc.size());
    return PHANT_OK;
}

// ---- transactions (src/types/transaction.zig, src/signer/signer.zig:81-188) ----
namespace {

struct TxItem {
    const uint8_t* full;  // the item with its header
    size_t total;
    const uint8_t* pay;
    size_t len;
    bool is_list;
};

// a big-endian integer of at most `max_bytes` bytes without a leading zero
bool tx_uint(const TxItem& it, size_t max_bytes) { return !it.is_list && it.len <= max_bytes && (it.len == 0 || it.pay[0] != 0); }

// [[address, [key, ...]], ...]
bool tx_access_list(const TxItem& al) {
    if (!al.is_list) return false;
    const uint8_t* p = al.pay;
    size_t left = al.len;
    while (left) {
        size_t pay, len, total;
        bool is_list;
        if (!host_rlp_item(p, left, pay, len, total, is_list) || !is_list) return false;
        const uint8_t* q = p + pay;
        size_t qleft = len, ip, il, it;
        bool ilist;
        if (!host_rlp_item(q, qleft, ip, il, it, ilist) || ilist || il != 20) return false;  // the address
        q += it, qleft -= it;
        if (!host_rlp_item(q, qleft, ip, il, it, ilist) || !ilist || it != qleft) return false;  // the keys, and nothing after
        const uint8_t* k = q + ip;
        size_t kleft = il;
        while (kleft) {
            size_t kp, kl, kt;
            bool klist;
            if (!host_rlp_item(k, kleft, kp, kl, kt, klist) || klist || kl != 32) return false;
            k += kt, kleft -= kt;
        }
        p += total, left -= total;
    }
    return true;
}

void put_list_header(std::vector<uint8_t>& out, size_t len) {
    uint8_t hdr[9];
    out.insert(out.end(), hdr, hdr + put_hdr(hdr, 0xc0u, len));
}

void pad32(uint8_t out[32], const TxItem& it) {
    std::memset(out, 0, 32);
    if (it.len) std::memcpy(out + 32 - it.len, it.pay, it.len);
}

}  // namespace

uint8_t tx_signing_parts(const uint8_t* tx, size_t len, uint64_t chain_id, std::vector<uint8_t>& preimage, uint8_t r[32],
                         uint8_t s[32], uint8_t* recid) {
    if (!tx || len == 0) return PHANT_SIG_BAD_TX;
    uint8_t type = 0;
    if (tx[0] < 0x80) {  // EIP-2718: a type byte in front of the list
        type = tx[0];
        if (type != 1 && type != 2) return PHANT_SIG_BAD_TX;
        ++tx, --len;
    }
    size_t pay, plen, total;
    bool is_list;
    if (!host_rlp_item(tx, len, pay, plen, total, is_list) || !is_list || total != len) return PHANT_SIG_BAD_TX;
    const size_t want = type == 0 ? 9 : type == 1 ? 11 : 12;
    TxItem it[12];
    size_t count = 0;
    const uint8_t* p = tx + pay;
    size_t left = plen;
    while (left) {
        size_t ip, il, tot;
        bool ilist;
        if (count == want || !host_rlp_item(p, left, ip, il, tot, ilist)) return PHANT_SIG_BAD_TX;
        it[count++] = TxItem{p, tot, p + ip, il, ilist};
        p += tot, left -= tot;
    }
    if (count != want) return PHANT_SIG_BAD_TX;
    // the fields of each type: widths as in src/types/transaction.zig; `to` empty (creation) or an address; data any string
    size_t to_i, data_i;
    if (type == 0) {  // nonce, gas_price, gas_limit, to, value, data, v, r, s
        if (!tx_uint(it[0], 8) || !tx_uint(it[1], 32) || !tx_uint(it[2], 8) || !tx_uint(it[4], 32)) return PHANT_SIG_BAD_TX;
        to_i = 3, data_i = 5;
    } else if (type == 1) {  // chain_id, nonce, gas_price, gas, to, value, data, access_list, y_parity, r, s
        if (!tx_uint(it[0], 8) || !tx_uint(it[1], 8) || !tx_uint(it[2], 32) || !tx_uint(it[3], 8) || !tx_uint(it[5], 32) ||
            !tx_access_list(it[7]))
            return PHANT_SIG_BAD_TX;
        to_i = 4, data_i = 6;
    } else {  // chain_id, nonce, max_priority_fee_per_gas, max_fee_per_gas, gas, to, value, data, access_list, y_parity, r, s
        if (!tx_uint(it[0], 8) || !tx_uint(it[1], 8) || !tx_uint(it[2], 32) || !tx_uint(it[3], 32) || !tx_uint(it[4], 8) ||
            !tx_uint(it[6], 32) || !tx_access_list(it[8]))
            return PHANT_SIG_BAD_TX;
        to_i = 5, data_i = 7;
    }
    if (it[to_i].is_list || (it[to_i].len != 0 && it[to_i].len != 20) || it[data_i].is_list) return PHANT_SIG_BAD_TX;
    const TxItem &v = it[want - 3], &ri = it[want - 2], &si = it[want - 1];
    if (!tx_uint(v, 32) || !tx_uint(ri, 32) || !tx_uint(si, 32)) return PHANT_SIG_BAD_TX;
    // v: a value of more than 9 bytes matches nothing below (35 + 2 chain_id + 1 < 2^66)
    unsigned __int128 vv = 0;
    if (v.len > 9) return PHANT_SIG_BAD_V;
    for (size_t k = 0; k < v.len; ++k) vv = vv << 8 | v.pay[k];
    bool eip155 = false;
    if (type == 0) {
        const unsigned __int128 base = (unsigned __int128)35 + 2 * (unsigned __int128)chain_id;
        if (vv == 27 || vv == 28) *recid = (uint8_t)(vv - 27);
        else if (vv == base || vv == base + 1) *recid = (uint8_t)(vv - base), eip155 = true;
        else return PHANT_SIG_BAD_V;
    } else {
        if (vv > 1) return PHANT_SIG_BAD_V;
        *recid = (uint8_t)vv;
    }
    pad32(r, ri);
    pad32(s, si);
    // the signed list: the items in front of v, verbatim, (chain_id, 0, 0 for EIP-155,) under a header of their own
    const size_t body = (size_t)(v.full - (tx + pay));
    uint8_t tail[12];
    size_t tail_len = 0;
    if (eip155) {
        tail_len = put_uint(tail, chain_id);
        tail[tail_len++] = 0x80;
        tail[tail_len++] = 0x80;
    }
    if (type) preimage.push_back(type);
    put_list_header(preimage, body + tail_len);
    preimage.insert(preimage.end(), tx + pay, tx + pay + body);
    preimage.insert(preimage.end(), tail, tail + tail_len);
    return PHANT_SIG_OK;
}

// ---- block headers (src/types/block.zig:15-69) ----
bool header_decode(const uint8_t* p, size_t len, bool from_block, const HeaderArrays& f, uint32_t i, uint32_t* extra_at) {
    uint8_t* const rows32[9] = {f.parent_hash, f.uncle_hash, f.state_root, f.transactions_root, f.receipts_root, f.prev_randao, f.withdrawals_root,
                                f.parent_beacon_root, f.requests_hash};
    uint64_t* const ints[7] = {f.difficulty, f.number, f.gas_limit, f.gas_used, f.timestamp, f.blob_gas_used, f.excess_blob_gas};
    for (uint8_t* r : rows32) std::memset(r + 32 * (size_t)i, 0, 32);
    for (uint64_t* v : ints) v[i] = 0;
    std::memset(f.fee_recipient + 20 * (size_t)i, 0, 20);
    std::memset(f.logs_bloom + 256 * (size_t)i, 0, 256);
    std::memset(f.nonce + 8 * (size_t)i, 0, 8);
    std::memset(f.base_fee + 32 * (size_t)i, 0, 32);
    f.n_fields[i] = 0;
    f.extra_off[i + 1] = *extra_at;
    if (!p) return false;
    size_t pay, plen, total;
    bool is_list;
    if (!host_rlp_item(p, len, pay, plen, total, is_list) || !is_list || total != len) return false;
    if (from_block) {  // [header, transactions, uncles, (withdrawals)]: the first item, the rest only walked
        const uint8_t* q = p + pay;
        size_t left = plen, hp = 0, hl = 0, ht = 0, count = 0;
        while (left) {
            size_t ip, il, it;
            bool ilist;
            if (!host_rlp_item(q, left, ip, il, it, ilist) || !ilist) return false;
            if (count == 0) hp = ip, hl = il, ht = it;
            ++count, q += it, left -= it;
        }
        if (count != 3 && count != 4) return false;
        p += pay, pay = hp, plen = hl, total = ht;
    }
    // the items: widths as in block.zig:15-36
    const uint8_t* item[21];
    size_t ilen[21], count = 0;
    const uint8_t* q = p + pay;
    size_t left = plen;
    while (left) {
        size_t ip, il, it;
        bool ilist;
        if (count == 21 || !host_rlp_item(q, left, ip, il, it, ilist) || ilist) return false;
        item[count] = q + ip, ilen[count] = il;
        ++count, q += it, left -= it;
    }
    if (count != 15 && count != 16 && count != 17 && count != 19 && count != 20 && count != 21) return false;
    static const uint16_t width[21] = {32, 32, 20, 32, 32, 32, 256, 0, 0, 0, 0, 0, 0, 32, 8, 0, 32, 0, 0, 32, 32};
    for (size_t k = 0; k < count; ++k) {
        const bool integer = (k >= 7 && k <= 11) || k == 15 || k == 17 || k == 18;
        if (integer ? (ilen[k] > (k == 15 ? 32u : 8u) || (ilen[k] && item[k][0] == 0)) : (k != 12 && ilen[k] != width[k])) return false;
    }
    if (ilen[12] > 0xffffffffull - *extra_at) return false;
    auto u64 = [&](size_t k) {
        uint64_t v = 0;
        for (size_t b = 0; b < ilen[k]; ++b) v = v << 8 | item[k][b];
        return v;
    };
    const size_t at32[9] = {0, 1, 3, 4, 5, 13, 16, 19, 20};
    for (size_t r = 0; r < 9; ++r)
        if (at32[r] < count) std::memcpy(rows32[r] + 32 * (size_t)i, item[at32[r]], 32);
    std::memcpy(f.fee_recipient + 20 * (size_t)i, item[2], 20);
    std::memcpy(f.logs_bloom + 256 * (size_t)i, item[6], 256);
    for (size_t k = 0; k < 5; ++k) ints[k][i] = u64(7 + k);
    if (ilen[12]) std::memcpy(f.extra_data + *extra_at, item[12], ilen[12]);
    *extra_at += (uint32_t)ilen[12];
    f.extra_off[i + 1] = *extra_at;
    std::memcpy(f.nonce + 8 * (size_t)i, item[14], 8);
    if (count >= 16 && ilen[15]) std::memcpy(f.base_fee + 32 * (size_t)i + 32 - ilen[15], item[15], ilen[15]);
    if (count >= 19) f.blob_gas_used[i] = u64(17), f.excess_blob_gas[i] = u64(18);
    f.n_fields[i] = (uint8_t)count;
    return true;
}

// ---- block bodies: [header,] transactions, uncles, (withdrawals) ----
// The items of the list payload p[0, len): `each(value, bytes)` for every one, given what `value_of` makes of it; false: an item that is
// not canonical RLP or that value_of refuses.
template <class ValueOf, class Each>
static bool walk_list(const uint8_t* p, size_t len, ValueOf&& value_of, Each&& each) {
    while (len) {
        size_t ip, il, it;
        bool ilist;
        if (!host_rlp_item(p, len, ip, il, it, ilist)) return false;
        const uint8_t* v;
        size_t vl;
        if (!value_of(p, ip, il, it, ilist, v, vl)) return false;
        each(v, vl);
        p += it, len -= it;
    }
    return true;
}

uint8_t body_split(const uint8_t* p, size_t len, bool has_header, BodyTotals& t, const BodySink* sink) {
    if (!p) return PHANT_SPLIT_BAD_RLP;
    size_t pay, plen, total;
    bool is_list;
    if (!host_rlp_item(p, len, pay, plen, total, is_list) || !is_list || total != len) return PHANT_SPLIT_BAD_RLP;
    // the outer items: every one a list
    const uint8_t* part[4];
    size_t part_len[4], count = 0;
    const uint8_t* q = p + pay;
    size_t left = plen;
    const size_t first = has_header ? 1 : 0;
    while (left) {
        size_t ip, il, it;
        bool ilist;
        if (count == first + 3 || !host_rlp_item(q, left, ip, il, it, ilist) || !ilist) return PHANT_SPLIT_BAD_RLP;
        part[count] = q + ip, part_len[count] = il;
        ++count, q += it, left -= it;
    }
    if (count != first + 2 && count != first + 3) return PHANT_SPLIT_BAD_RLP;
    const uint8_t* const txs = part[first];
    const size_t txs_len = part_len[first];
    const bool has_wd = count == first + 3;
    // a transaction: a list as it stands, or the payload of a string that begins with a type byte
    auto tx_value = [](const uint8_t* item, size_t ip, size_t il, size_t it, bool ilist, const uint8_t*& v, size_t& vl) {
        if (ilist) return v = item, vl = it, true;
        if (il == 0 || item[ip] > 0x7fu) return false;
        return v = item + ip, vl = il, true;
    };
    auto wd_value = [](const uint8_t* item, size_t, size_t, size_t it, bool ilist, const uint8_t*& v, size_t& vl) { return v = item, vl = it, ilist; };
    BodyTotals mine{0, 0, 0, 0};
    // (which of the two a false means: walk once more for the RLP alone)
    auto any_value = [](const uint8_t* item, size_t, size_t, size_t it, bool, const uint8_t*& v, size_t& vl) { return v = item, vl = it, true; };
    auto nothing = [](const uint8_t*, size_t) {};
    if (!walk_list(txs, txs_len, tx_value, [&](const uint8_t*, size_t vl) { ++mine.n, mine.tx_bytes += vl; }))
        return walk_list(txs, txs_len, any_value, nothing) ? PHANT_SPLIT_BAD_TX : PHANT_SPLIT_BAD_RLP;
    if (part_len[first + 1] != 0) return PHANT_SPLIT_UNCLES;
    if (has_wd && !walk_list(part[first + 2], part_len[first + 2], wd_value, [&](const uint8_t*, size_t vl) { ++mine.n_wd, mine.wd_bytes += vl; }))
        return walk_list(part[first + 2], part_len[first + 2], any_value, nothing) ? PHANT_SPLIT_BAD_WITHDRAWAL : PHANT_SPLIT_BAD_RLP;
    if (sink) {
        uint64_t i = t.n, at = t.tx_bytes;
        (void)walk_list(txs, txs_len, tx_value, [&](const uint8_t* v, size_t vl) {
            std::memcpy(sink->txs + at, v, vl);
            at += vl;
            sink->tx_off[++i] = at;
        });
        i = t.n_wd, at = t.wd_bytes;
        if (has_wd)
            (void)walk_list(part[first + 2], part_len[first + 2], wd_value, [&](const uint8_t* v, size_t vl) {
                std::memcpy(sink->wd + at, v, vl);
                at += vl;
                sink->wd_off[++i] = at;
            });
    }
    t.n += mine.n, t.n_wd += mine.n_wd, t.tx_bytes += mine.tx_bytes, t.wd_bytes += mine.wd_bytes;
    return PHANT_SPLIT_OK;
}

// ---- the per-block element of a `Receipts` message: the list of the block's receipts ----
uint8_t receipts_split(const uint8_t* p, size_t len, bool eth69, ReceiptTotals& t, const ReceiptSink* sink) {
    if (!p) return PHANT_SPLIT_BAD_RLP;
    size_t pay, plen, total;
    bool is_list;
    if (!host_rlp_item(p, len, pay, plen, total, is_list) || !is_list || total != len) return PHANT_SPLIT_BAD_RLP;
    // a receipt: a list as it stands, or (before eth/69) the payload of a string that begins with a type byte
    auto value = [eth69](const uint8_t* item, size_t ip, size_t il, size_t it, bool ilist, const uint8_t*& v, size_t& vl) {
        if (ilist) return v = item, vl = it, true;
        if (eth69 || il == 0 || item[ip] > 0x7fu) return false;
        return v = item + ip, vl = il, true;
    };
    auto any_value = [](const uint8_t* item, size_t, size_t, size_t it, bool, const uint8_t*& v, size_t& vl) { return v = item, vl = it, true; };
    ReceiptTotals mine{0, 0};
    if (!walk_list(p + pay, plen, value, [&](const uint8_t*, size_t vl) { ++mine.n, mine.bytes += vl; }))
        return walk_list(p + pay, plen, any_value, [](const uint8_t*, size_t) {}) ? PHANT_SPLIT_BAD_RECEIPT : PHANT_SPLIT_BAD_RLP;
    if (sink) {
        uint64_t i = t.n, at = t.bytes;
        (void)walk_list(p + pay, plen, value, [&](const uint8_t* v, size_t vl) {
            std::memcpy(sink->receipts + at, v, vl);
            at += vl;
            sink->rc_off[++i] = at;
        });
    }
    t.n += mine.n, t.bytes += mine.bytes;
    return PHANT_SPLIT_OK;
}

}  // namespace phant
