// db_args.h -- the host-side half of db.hip: the walk over a database file's
// header and record frames (syzsig_db_scan's body, pkg/db/db.go:203-265 without
// the inflate) and what the device entry points reject before any device work.
// No HIP here, so that tests/db_driver.cc runs every branch on the CPU under
// ASan + UBSan.  Whoever includes this has syzsig.h's codes.
#pragma once

#include <cstdint>

#include "sigs_args.h"

namespace syz {

constexpr uint32_t kDbMagic = 0xbaddb, kDbRecMagic = 0xfee1bad, kDbCurVersion = 2;  // db.go:134-139
constexpr uint64_t kDbSeqDeleted = ~0ull;
constexpr uint64_t kInflateMaxBatch = 1ull << 25;  // streams of one call, as a batch of Sigs

// data[at .. at + 4) / [at .. at + 8) little-endian (binary.LittleEndian); the caller checked the range
inline uint32_t db_u32(const uint8_t* p, uint64_t at)
{
	return p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
}
inline uint64_t db_u64(const uint8_t* p, uint64_t at) { return db_u32(p, at) | (uint64_t)db_u32(p, at + 4) << 32; }

struct DbScan {
	uint64_t version = 0, n = 0;
	uint32_t ended = SYZSIG_DB_END_EOF;
};

// The walk.  Every length is compared with the bytes left (nbytes - at, which
// cannot wrap: at <= nbytes throughout), never added to an offset first.  With
// the arrays given (all five, room for the records this walk finds) they are
// filled; nullptr: counted only.
inline DbScan db_scan(const uint8_t* data, uint64_t nbytes, uint64_t* key_off, uint32_t* key_len, uint64_t* seq,
                      uint64_t* val_off, uint32_t* val_len)
{
	DbScan r;
	if (nbytes == 0)
		return r;  // db.go:206-208: the empty file is version 0 and no error
	uint64_t at = 0;
	r.ended = SYZSIG_DB_END_BAD_HEADER;
	if (nbytes < 8 || db_u32(data, 0) != kDbMagic)
		return r;
	const uint32_t ver = db_u32(data, 4);
	if (ver == 0 || ver > kDbCurVersion)
		return r;
	at = 8;
	if (ver >= 2) {
		if (nbytes - at < 8)
			return r;
		r.version = db_u64(data, at);
		at += 8;
	}
	for (;;) {
		if (at == nbytes) {
			r.ended = SYZSIG_DB_END_EOF;  // db.go:187-189: io.EOF at a record's first byte
			return r;
		}
		r.ended = SYZSIG_DB_END_TRUNCATED;
		if (nbytes - at < 4)
			return r;
		if (db_u32(data, at) != kDbRecMagic) {
			r.ended = SYZSIG_DB_END_BAD_MAGIC;
			return r;
		}
		at += 4;
		if (nbytes - at < 4)
			return r;
		const uint32_t kl = db_u32(data, at);
		at += 4;
		if (nbytes - at < kl)
			return r;
		const uint64_t ko = at;
		at += kl;
		if (nbytes - at < 8)
			return r;
		const uint64_t sq = db_u64(data, at);
		at += 8;
		uint64_t vo = 0;
		uint32_t vl = 0;
		if (sq != kDbSeqDeleted) {
			if (nbytes - at < 4)
				return r;
			vl = db_u32(data, at);
			at += 4;
			if (nbytes - at < vl)
				return r;
			vo = vl ? at : 0;
			at += vl;
		}
		if (key_off) {
			key_off[r.n] = ko;
			key_len[r.n] = kl;
			seq[r.n] = sq;
			val_off[r.n] = vo;
			val_len[r.n] = vl;
		}
		r.n++;
	}
}

inline ArgStatus db_scan_args(const uint8_t* data, uint64_t nbytes, const uint64_t* version, const uint64_t* n,
                              const uint32_t* ended)
{
	if (!version || !n || !ended || (nbytes && !data))
		return ArgStatus{SYZSIG_EINVAL, "db_scan: NULL argument"};
	return arg_ok();
}

// ... once the records are counted: `cap` entries of room in the five arrays
inline ArgStatus db_scan_room(uint64_t n, uint64_t cap, bool arrays)
{
	if (n > cap)
		return ArgStatus{SYZSIG_ERANGE, "db_scan: more records than cap"};
	if (n && !arrays)
		return ArgStatus{SYZSIG_EINVAL, "db_scan: NULL output"};
	return arg_ok();
}

// syzsig_inflate_dev before the ranges are looked at (they are device memory)
inline ArgStatus inflate_args(const void* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                              const uint32_t* d_src_len, uint64_t n, const uint8_t* d_out, uint64_t out_cap,
                              const uint64_t* d_out_off, const uint8_t* d_status, const uint64_t* out_bytes)
{
	if (!ctx)
		return ArgStatus{SYZSIG_EINVAL, "inflate: NULL context"};
	if (!out_bytes || !d_out_off)
		return ArgStatus{SYZSIG_EINVAL, "inflate: NULL argument"};
	if (n > kInflateMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "inflate: more than 2^25 streams in one call"};
	if (n && (!d_src_off || !d_src_len || !d_status || (nbytes && !d_src)))
		return ArgStatus{SYZSIG_EINVAL, "inflate: NULL argument"};
	if (!d_out && out_cap)
		return ArgStatus{SYZSIG_EINVAL, "inflate: NULL output with a capacity"};
	return arg_ok();
}

// ... and after: `bad` ranges that pass nbytes
inline ArgStatus inflate_ranges_status(uint64_t bad)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "inflate: a stream's range passes nbytes"};
	return arg_ok();
}

// ... and once the total is known.  sizing = a NULL d_out: the lengths and statuses only.
inline ArgStatus inflate_room(uint64_t total, uint64_t out_cap, bool sizing)
{
	if (!sizing && total > out_cap)
		return ArgStatus{SYZSIG_ERANGE, "inflate: the output is longer than out_cap"};
	return arg_ok();
}

// syzsig_deflate_dev before the ranges are looked at
inline ArgStatus deflate_args(const void* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                              const uint32_t* d_src_len, uint64_t n, const uint8_t* d_out, uint64_t out_cap,
                              const uint64_t* d_out_off, const uint64_t* out_bytes)
{
	if (!ctx)
		return ArgStatus{SYZSIG_EINVAL, "deflate: NULL context"};
	if (!out_bytes || !d_out_off)
		return ArgStatus{SYZSIG_EINVAL, "deflate: NULL argument"};
	if (n > kInflateMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "deflate: more than 2^25 values in one call"};
	if (n && (!d_src_off || !d_src_len || (nbytes && !d_src)))
		return ArgStatus{SYZSIG_EINVAL, "deflate: NULL argument"};
	if (!d_out && out_cap)
		return ArgStatus{SYZSIG_EINVAL, "deflate: NULL output with a capacity"};
	return arg_ok();
}

// ... and after: `bad` ranges that pass nbytes, `huge` values past SYZSIG_INFLATE_MAX_OUT
inline ArgStatus deflate_ranges_status(uint64_t bad, uint64_t huge)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "deflate: a value's range passes nbytes"};
	if (huge)
		return ArgStatus{SYZSIG_ERANGE, "deflate: a value is longer than SYZSIG_INFLATE_MAX_OUT"};
	return arg_ok();
}

// ... and once the total is known (deflate and db_records).  sizing = a NULL d_out.
inline ArgStatus write_room(uint64_t total, uint64_t out_cap, bool sizing, const char* who_range)
{
	if (!sizing && total > out_cap)
		return ArgStatus{SYZSIG_ERANGE, who_range};
	return arg_ok();
}

// syzsig_deflate_host, before the value is read
inline ArgStatus deflate_host_args(const uint8_t* src, uint64_t len, const uint8_t* out, uint64_t cap,
                                   const uint64_t* out_len, uint64_t max_len)
{
	if (!out_len || (len && !src) || (cap && !out))
		return ArgStatus{SYZSIG_EINVAL, "deflate_host: NULL argument"};
	if (len > max_len)
		return ArgStatus{SYZSIG_ERANGE, "deflate_host: the value is longer than SYZSIG_INFLATE_MAX_OUT"};
	return arg_ok();
}

// syzsig_db_records_dev before the offsets are looked at
inline ArgStatus db_records_args(const void* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n,
                                 const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_stream_off,
                                 const uint8_t* d_out, uint64_t out_cap, const uint64_t* d_rec_off,
                                 const uint64_t* out_bytes)
{
	if (!ctx || !out_bytes || !d_rec_off)
		return ArgStatus{SYZSIG_EINVAL, "db_records: NULL argument"};
	if (n > kSigsMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "db_records: more than 2^25 records in one call"};
	if (n && (!d_sig || !d_seq || !d_stream_off || (stream_bytes && !d_stream)))
		return ArgStatus{SYZSIG_EINVAL, "db_records: NULL argument"};
	if (!d_out && out_cap)
		return ArgStatus{SYZSIG_EINVAL, "db_records: NULL output with a capacity"};
	return arg_ok();
}

// ... and after: offsets that decrease or pass stream_bytes, deletes that carry a stream, streams of 2^32 bytes
inline ArgStatus db_records_status(uint64_t bad, uint64_t del_with_val, uint64_t huge)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "db_records: the stream offsets decrease or pass stream_bytes"};
	if (del_with_val)
		return ArgStatus{SYZSIG_EINVAL, "db_records: deleting record with value"};
	if (huge)
		return ArgStatus{SYZSIG_ERANGE, "db_records: a stream of 2^32 bytes or more"};
	return arg_ok();
}

// syzsig_db_apply_dev before anything on the device is looked at
inline ArgStatus db_apply_args(const void* ctx, const uint8_t* d_live_sig, const uint64_t* d_live_seq, uint64_t nl,
                               const uint8_t* d_live_data, uint64_t live_bytes, const uint64_t* d_live_off,
                               const uint8_t* d_op_sig, const uint64_t* d_op_seq, uint64_t m, const uint8_t* d_op_data,
                               uint64_t op_bytes, const uint64_t* d_op_off, const uint8_t* d_written,
                               const uint8_t* d_keep_live, const uint8_t* d_keep_op, const uint64_t* nwritten,
                               const uint64_t* nkeep_live, const uint64_t* nkeep_op)
{
	if (!ctx || !nwritten || !nkeep_live || !nkeep_op)
		return ArgStatus{SYZSIG_EINVAL, "db_apply: NULL argument"};
	if (nl > kSigsMaxBatch || m > kSigsMaxBatch || nl + m > kSigsMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "db_apply: more than 2^25 records and ops in one call"};
	if (nl && (!d_live_sig || !d_live_seq || !d_live_off || !d_keep_live || (live_bytes && !d_live_data)))
		return ArgStatus{SYZSIG_EINVAL, "db_apply: NULL argument"};
	if (m && (!d_op_sig || !d_op_seq || !d_op_off || !d_written || !d_keep_op || (op_bytes && !d_op_data)))
		return ArgStatus{SYZSIG_EINVAL, "db_apply: NULL argument"};
	return arg_ok();
}

// ... and after: offsets that decrease or pass their nbytes, deletes with a value, live seqs of ^0
inline ArgStatus db_apply_status(uint64_t bad, uint64_t del_with_val, uint64_t live_deleted)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "db_apply: the offsets decrease or pass their nbytes"};
	if (del_with_val)
		return ArgStatus{SYZSIG_EINVAL, "db_apply: deleting record with value"};
	if (live_deleted)
		return ArgStatus{SYZSIG_EINVAL, "db_apply: a live record with the reserved seq"};
	return arg_ok();
}

inline ArgStatus db_live_args(const void* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n, uint64_t nvalid,
                              const uint8_t* d_live, const uint64_t* nlive, const uint64_t* uncompacted)
{
	if (!ctx || !nlive || !uncompacted)
		return ArgStatus{SYZSIG_EINVAL, "db_live: NULL argument"};
	if (n > kSigsMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "db_live: more than 2^25 records in one call"};
	if (nvalid > n)
		return ArgStatus{SYZSIG_EINVAL, "db_live: nvalid is more than n"};
	if (n && (!d_sig || !d_seq || !d_live))
		return ArgStatus{SYZSIG_EINVAL, "db_live: NULL argument"};
	return arg_ok();
}

}  // namespace syz
