// db.hip -- pkg/db's read side: the frames of a database file on the host
// (syzsig_db_scan) and its values through a batched RFC 1951 decoder on the
// device (syzsig_inflate_dev).  The map's last-write-wins, syzsig_db_live_dev, is
// the third client of the Sig sets' sort and lives next to it in sigs.hip.
// Behind it the write side: a batched compressor (syzsig_deflate_dev,
// syzsig_deflate_host) and serializeRecord's frames (syzsig_db_records_dev).
//
// References:
//   pkg/db/db.go:177-200   deserializeDB: the header, then records until io.EOF
//       or the first error; a delete removes the key, anything else overwrites
//   pkg/db/db.go:203-227   deserializeHeader
//   pkg/db/db.go:229-265   deserializeRecord: magic, key, seq, valLen, and
//       flate.NewReader over valLen bytes read until the final block
//   pkg/db/db.go:164-172   the writer's stream: data blocks, an empty stored
//       block (Flush), an empty final stored block (Close)
//
// Inflate.  DEFLATE is serial inside a stream, so a lane owns a stream, as a
// lane owns a message in sigs.hip, and a workgroup is one wave:
//   k_inf_prep    per stream: its range checked against nbytes (nothing else
//                 runs when one is bad), the streams longer than kInfLong listed
//   k_inf_wave<W> stream 64 b + lane, skipping the listed and the empty ones.
//                 W = false, the counting pass: the decoder of inflate_core.h
//                 without an output, which gives the status and the length;
//                 W = true, after the lengths are scanned into offsets: the same
//                 decode of the OK streams into d_out at their offsets, each
//                 write bounded by the stream's counted extent.
//   k_inf_long<W> the list, one stream per lane
//   k_inf_scan    lengths -> offsets, one workgroup, chunk by chunk with a carry
// The tables of a lane (inflate_core.h: 368 16-bit cells) are in LDS, cell c of
// lane l at [c * 64 + l], so that the lanes of a wave that are at the same cell
// touch 32 consecutive words: 46 KiB per wave, three waves per CU.  A match is
// copied byte by byte from the stream's own output in global memory.  No kernel
// waits for another wave; every loop is bounded by the stream's bits.
#include <algorithm>

#include "segsort.h"
// (after segsort.h: the two below take syzsig.h's codes from their includer)
#include "db_args.h"
#include "inflate_core.h"

namespace syz {

constexpr uint32_t kInfLong = SYZSIG_INFLATE_LONG;
constexpr int kIfShort = kCntInserted, kIfLong = kCntTouched, kIfStored = kCntChanged, kIfFixed = kCntCandidates,
              kIfDynamic = kCntAux;
static_assert(kInfTabCells * 64 * 2 <= 64 * 1024, "one wave's tables are static LDS");
static_assert(kInfOk == SYZSIG_INFLATE_OK && kInfTruncated == SYZSIG_INFLATE_TRUNCATED &&
                  kInfInvalid == SYZSIG_INFLATE_INVALID && kInfTrailing == SYZSIG_INFLATE_TRAILING &&
                  kInfTooLong == SYZSIG_INFLATE_TOO_LONG,
              "inflate_core.h restates the header's statuses");

// one lane's tables inside the wave's LDS block
struct InfTabLds {
	uint16_t* base;  // + lane
	__device__ __forceinline__ uint32_t get(int i) const { return base[i * 64]; }
	__device__ __forceinline__ void set(int i, uint32_t v) { base[i * 64] = (uint16_t)v; }
};

// Per stream: its range checked; longer than kInfLong: listed.
__global__ __launch_bounds__(256) void k_inf_prep(const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                  uint64_t n, uint64_t nbytes, uint32_t* list, uint64_t list_cap,
                                                  unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
		const uint64_t a = off[i], l = len[i];
		if (l == 0)
			continue;  // (skipped whatever its offset says)
		if (a > nbytes || l > nbytes - a) {
			bad++;
			continue;
		}
		if (l > kInfLong) {
			const uint64_t x = atomicAdd(&cnt[kIfLong], 1ull);
			if (x < list_cap)  // (streams past kInfLong bytes inside nbytes: cannot fail for valid ranges)
				list[x] = (uint32_t)i;
		}
	}
	block_count(&cnt[kCntError], bad);
}

// Stream i on this lane.  Counting: status[i] and olen[i] are set.  Writing:
// the OK streams' bytes to out + ooff[i], at most olen[i] of them.
template <bool kWrite>
__device__ __forceinline__ void inf_one(const uint8_t* __restrict__ src, uint64_t a, uint64_t l, uint64_t i,
                                        uint8_t* status, uint32_t* olen, const uint64_t* __restrict__ ooff,
                                        uint8_t* out, InfTabLds& t, uint64_t (&blocks)[3])
{
	if (kWrite) {
		if (status[i] != kInfOk || olen[i] == 0)
			return;
		(void)inflate_stream(src + a, l, out + ooff[i], olen[i], SYZSIG_INFLATE_MAX_OUT, t);
	} else {
		const InflateResult r = inflate_stream(src + a, l, nullptr, 0, SYZSIG_INFLATE_MAX_OUT, t);
		status[i] = r.status;
		olen[i] = r.status == kInfOk ? (uint32_t)r.out_len : 0;
		blocks[0] += r.stored;
		blocks[1] += r.fixed;
		blocks[2] += r.dynamic;
	}
}

__device__ __forceinline__ void inf_count(unsigned long long* cnt, uint64_t mine, int path, uint64_t (&blocks)[3])
{
	const uint64_t nmine = wave_sum_u64(mine), s = wave_sum_u64(blocks[0]), f = wave_sum_u64(blocks[1]),
	               d = wave_sum_u64(blocks[2]);
	if (threadIdx.x == 0) {
		if (nmine)
			atomicAdd(&cnt[path], (unsigned long long)nmine);
		if (s)
			atomicAdd(&cnt[kIfStored], (unsigned long long)s);
		if (f)
			atomicAdd(&cnt[kIfFixed], (unsigned long long)f);
		if (d)
			atomicAdd(&cnt[kIfDynamic], (unsigned long long)d);
	}
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_inf_wave(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, uint64_t n, uint8_t* status,
                                                 uint32_t* olen, const uint64_t* __restrict__ ooff, uint8_t* out,
                                                 unsigned long long* cnt)
{
	__shared__ uint16_t tabs[kInfTabCells * 64];
	InfTabLds t{tabs + threadIdx.x};
	const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	uint64_t blocks[3] = {0, 0, 0};
	bool mine = false;
	if (i < n) {
		const uint64_t l = len[i];
		if (l == 0 && !kWrite) {
			status[i] = kInfOk;
			olen[i] = 0;
		}
		mine = l != 0 && l <= kInfLong;
		if (mine)
			inf_one<kWrite>(src, off[i], l, i, status, olen, ooff, out, t, blocks);
	}
	if (!kWrite)
		inf_count(cnt, mine, kIfShort, blocks);
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_inf_long(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, const uint32_t* __restrict__ list,
                                                 uint64_t nlong, uint8_t* status, uint32_t* olen,
                                                 const uint64_t* __restrict__ ooff, uint8_t* out,
                                                 unsigned long long* cnt)
{
	__shared__ uint16_t tabs[kInfTabCells * 64];
	InfTabLds t{tabs + threadIdx.x};
	const uint64_t x = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	uint64_t blocks[3] = {0, 0, 0};
	if (x < nlong) {
		const uint64_t i = list[x];
		inf_one<kWrite>(src, off[i], len[i], i, status, olen, ooff, out, t, blocks);
	}
	if (!kWrite)
		inf_count(cnt, 0, kIfShort, blocks);
}

// ooff[i] = olen[0] + ... + olen[i - 1], i <= n: one workgroup, 256 entries at a time
template <class Len>
__global__ __launch_bounds__(256) void k_inf_scan(const Len* __restrict__ olen, uint64_t n, uint64_t* ooff)
{
	__shared__ uint64_t s_w[4];
	uint64_t carry = 0;
	for (uint64_t base = 0; base < n; base += 256) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t x = i < n ? olen[i] : 0;
		uint64_t incl = x;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const uint64_t y = __shfl_up(incl, o, 64);
			if ((int)lane_id() >= o)
				incl += y;
		}
		__syncthreads();  // the last chunk's sums are read
		if (lane_id() == 63)
			s_w[threadIdx.x >> 6] = incl;
		__syncthreads();
		uint64_t wb = 0, total = 0;
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			wb += k < (threadIdx.x >> 6) ? s_w[k] : 0;
			total += s_w[k];
		}
		if (i < n)
			ooff[i] = carry + wb + incl - x;
		carry += total;
	}
	if (threadIdx.x == 0)
		ooff[n] = carry;
}

static int db_arg_fail(const ArgStatus& a) { return fail(a.code, a.msg); }

#define SYZ_DB_ARGS(expr)                                                          \
	do {                                                                           \
		const syz::ArgStatus a__ = (expr);                                         \
		if (a__.code != SYZSIG_OK)                                                 \
			return syz::db_arg_fail(a__);                                          \
	} while (0)

}  // namespace syz

using namespace syz;

extern "C" int syzsig_db_scan(const uint8_t* data, uint64_t nbytes, uint64_t cap, uint64_t* version, uint64_t* n,
                              uint32_t* ended, uint64_t* key_off, uint32_t* key_len, uint64_t* seq, uint64_t* val_off,
                              uint32_t* val_len)
{
	if (n)
		*n = 0;
	SYZ_DB_ARGS(db_scan_args(data, nbytes, version, n, ended));
	const DbScan r = db_scan(data, nbytes, nullptr, nullptr, nullptr, nullptr, nullptr);
	*n = r.n;
	SYZ_DB_ARGS(db_scan_room(r.n, cap, key_off && key_len && seq && val_off && val_len));
	if (r.n)
		(void)db_scan(data, nbytes, key_off, key_len, seq, val_off, val_len);
	*version = r.version;
	*ended = r.ended;
	return SYZSIG_OK;
}

extern "C" int syzsig_inflate_dev(syzsig_ctx* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                                  const uint32_t* d_src_len, uint64_t n, uint8_t* d_out, uint64_t out_cap,
                                  uint64_t* d_out_off, uint8_t* d_status, uint64_t* out_bytes)
{
	SYZ_LOCK(ctx);
	if (out_bytes)
		*out_bytes = 0;
	SYZ_DB_ARGS(inflate_args(ctx, d_src, nbytes, d_src_off, d_src_len, n, d_out, out_cap, d_out_off, d_status,
	                         out_bytes));
	std::fill(ctx->if_stats, ctx->if_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	if (n == 0) {
		SYZ_HIP(hipMemsetAsync(d_out_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const uint64_t list_cap = std::min<uint64_t>(n, nbytes / (kInfLong + 1)) + 1;
	uint32_t* list;
	char* meta;  // the outputs held back: status[n], then olen[n], then ooff[n + 1]
	const size_t o_len = align256(n), o_off = o_len + align256(n * 4);
	SYZ_TRY(ws_get(ctx, kWsInfList, list_cap * 4, (void**)&list));
	SYZ_TRY(ws_get(ctx, kWsInfMeta, o_off + (n + 1) * 8, (void**)&meta));
	uint8_t* status = (uint8_t*)meta;
	uint32_t* olen = (uint32_t*)(meta + o_len);
	uint64_t* ooff = (uint64_t*)(meta + o_off);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_inf_prep<<<grid_for(n, 256), 256, 0, s>>>(d_src_off, d_src_len, n, nbytes, list, list_cap, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_DB_ARGS(inflate_ranges_status(ctx->h_cnt[kCntError]));
	const uint64_t nlong = ctx->h_cnt[kIfLong];
	if (nlong >= list_cap)
		return fail(SYZSIG_EIO, "inflate: internal: more long streams than nbytes holds");
	const unsigned waves = (unsigned)((n + 63) / 64), lwaves = (unsigned)((nlong + 63) / 64);
	k_inf_wave<false><<<waves, 64, 0, s>>>(d_src, d_src_off, d_src_len, n, status, olen, nullptr, nullptr, ctx->d_cnt);
	if (nlong)
		k_inf_long<false><<<lwaves, 64, 0, s>>>(d_src, d_src_off, d_src_len, list, nlong, status, olen, nullptr, nullptr,
		                                       ctx->d_cnt);
	k_inf_scan<uint32_t><<<1, 256, 0, s>>>(olen, n, ooff);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, ooff + n, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	*out_bytes = total;
	ctx->if_stats[0] = ctx->h_cnt[kIfShort];
	ctx->if_stats[1] = nlong;
	ctx->if_stats[2] = ctx->h_cnt[kIfStored];
	ctx->if_stats[3] = ctx->h_cnt[kIfFixed] | ctx->h_cnt[kIfDynamic] << 32;
	SYZ_DB_ARGS(inflate_room(total, out_cap, d_out == nullptr));
	if (d_out && total) {
		k_inf_wave<true><<<waves, 64, 0, s>>>(d_src, d_src_off, d_src_len, n, status, olen, ooff, d_out, ctx->d_cnt);
		if (nlong)
			k_inf_long<true><<<lwaves, 64, 0, s>>>(d_src, d_src_off, d_src_len, list, nlong, status, olen, ooff, d_out,
			                                      ctx->d_cnt);
		SYZ_HIP(hipGetLastError());
	}
	SYZ_HIP(hipMemcpyAsync(d_out_off, ooff, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipMemcpyAsync(d_status, status, n, hipMemcpyDeviceToDevice, s));
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_inflate_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::if_stats, out, "inflate_stats");
}

// ---- the write side ----
//
// References:
//   pkg/db/db.go:147-175   serializeRecord: magic, key, seq, and unless the
//       record is a delete valLen and the value's DEFLATE stream
//   pkg/db/db.go:55-74     Save / Delete: syzsig_db_apply_dev, in sigs.hip
//
// Deflate is the inflater's mapping turned round: a lane owns a value, a
// workgroup is one wave, and deflate_core.h's compressor runs twice:
//   k_def_prep    per value: its range checked against nbytes and its length
//                 against SYZSIG_INFLATE_MAX_OUT (nothing else runs when one
//                 fails), the values longer than kDefLong listed
//   k_def_wave<W> value 64 b + lane, skipping the listed and the empty ones.
//                 W = false: the compressor without an output, which gives the
//                 stream's length and form; W = true, after k_inf_scan: the
//                 same search again, the stream written at its offset, each
//                 byte bounded by the counted extent.  A value that goes out
//                 stored is recognised by its counted length and not searched
//                 a second time.
//   k_def_long<W> the list, one value per lane
// A lane's hash table (deflate_core.h: 512 16-bit cells) is in LDS, cell c of
// lane l at [c * 64 + l]: 64 KiB per wave, two waves per CU.  The table is
// cleared by its lane before the first byte, so a stream never depends on what
// another value left there.
// Frames:
//   k_rec_len     a record's length from its seq and its stream's length; the
//                 offsets, a delete with a stream, a stream of 2^32 bytes counted
//   k_rec_write   one wave per record: the frame's bytes, one per lane, then the
//                 stream copied 64 bytes at a time

#include "deflate_core.h"

namespace syz {

constexpr uint32_t kDefLong = SYZSIG_DEFLATE_LONG;
static_assert(kDefTabCells * 64 * 2 <= 64 * 1024, "one wave's hash tables are static LDS");

// one lane's hash table inside the wave's LDS block
struct DefTabLds {
	uint16_t* base;  // + lane
	__device__ __forceinline__ uint32_t get(int i) const { return base[i * 64]; }
	__device__ __forceinline__ void set(int i, uint32_t v) { base[i * 64] = (uint16_t)v; }
};

// Per value: its range checked (nothing else runs when one is bad or too
// long); longer than kDefLong: listed.
__global__ __launch_bounds__(256) void k_def_prep(const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                  uint64_t n, uint64_t nbytes, uint32_t* list, uint64_t list_cap,
                                                  unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0, huge = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
		const uint64_t a = off[i], l = len[i];
		if (l == 0)
			continue;  // (skipped whatever its offset says)
		if (a > nbytes || l > nbytes - a) {
			bad++;
			continue;
		}
		if (l > SYZSIG_INFLATE_MAX_OUT) {
			huge++;
		} else if (l > kDefLong) {
			const uint64_t x = atomicAdd(&cnt[kIfLong], 1ull);
			if (x < list_cap)  // (values past kDefLong bytes inside nbytes: cannot fail for valid ranges)
				list[x] = (uint32_t)i;
		}
	}
	block_count(&cnt[kCntError], bad);
	block_count(&cnt[kIfDynamic], huge);
}

// Value i on this lane.  Counting: olen[i] is set.  Writing: the stream to
// out + ooff[i], at most olen[i] bytes of it.
template <bool kWrite>
__device__ __forceinline__ void def_one(const uint8_t* __restrict__ src, uint64_t a, uint64_t l, uint64_t i,
                                        uint32_t* olen, const uint64_t* __restrict__ ooff, uint8_t* out, DefTabLds& t,
                                        uint64_t (&forms)[2])
{
	if (kWrite) {
		(void)deflate_stream(src + a, l, out + ooff[i], olen[i], olen[i], t);
	} else {
		const DeflateResult r = deflate_stream(src + a, l, nullptr, 0, 0, t);
		olen[i] = (uint32_t)r.out_len;  // (at most 2^28 + 5 * 4097)
		forms[r.stored ? 0 : 1]++;
	}
}

__device__ __forceinline__ void def_count(unsigned long long* cnt, uint64_t mine, uint64_t (&forms)[2])
{
	const uint64_t nmine = wave_sum_u64(mine), s = wave_sum_u64(forms[0]), f = wave_sum_u64(forms[1]);
	if (threadIdx.x == 0) {
		if (nmine)
			atomicAdd(&cnt[kIfShort], (unsigned long long)nmine);
		if (s)
			atomicAdd(&cnt[kIfStored], (unsigned long long)s);
		if (f)
			atomicAdd(&cnt[kIfFixed], (unsigned long long)f);
	}
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_def_wave(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, uint64_t n, uint32_t* olen,
                                                 const uint64_t* __restrict__ ooff, uint8_t* out,
                                                 unsigned long long* cnt)
{
	__shared__ uint16_t tabs[kDefTabCells * 64];
	DefTabLds t{tabs + threadIdx.x};
	const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	uint64_t forms[2] = {0, 0};
	bool mine = false;
	if (i < n) {
		const uint64_t l = len[i];
		if (l == 0 && !kWrite)
			olen[i] = 0;
		mine = l != 0 && l <= kDefLong;
		if (mine)
			def_one<kWrite>(src, off[i], l, i, olen, ooff, out, t, forms);
	}
	if (!kWrite)
		def_count(cnt, mine, forms);
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_def_long(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, const uint32_t* __restrict__ list,
                                                 uint64_t nlong, uint32_t* olen, const uint64_t* __restrict__ ooff,
                                                 uint8_t* out, unsigned long long* cnt)
{
	__shared__ uint16_t tabs[kDefTabCells * 64];
	DefTabLds t{tabs + threadIdx.x};
	const uint64_t x = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	uint64_t forms[2] = {0, 0};
	if (x < nlong) {
		const uint64_t i = list[x];
		def_one<kWrite>(src, off[i], len[i], i, olen, ooff, out, t, forms);
	}
	if (!kWrite)
		def_count(cnt, 0, forms);
}

// Record i's length from its seq and its stream's: 56 for a delete, else 60 +
// the stream; the offsets checked on the way.
__global__ __launch_bounds__(256) void k_rec_len(const uint64_t* __restrict__ seq, const uint64_t* __restrict__ soff,
                                                 uint64_t n, uint64_t sbytes, uint64_t* rlen, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0, delv = 0, huge = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
		const uint64_t a = soff[i], b = soff[i + 1];
		uint64_t l = 0;
		if (a > b || b > sbytes)
			bad++;
		else if (seq[i] == kDbSeqDeleted)
			delv += b != a;
		else if (b - a >= 1ull << 32)
			huge++;
		else
			l = b - a + 4;
		rlen[i] = 56 + l;
	}
	block_count(&cnt[kCntError], bad);
	block_count(&cnt[kCntAux], delv);
	block_count(&cnt[kCntTouched], huge);
}

// One wave per record: its 56 or 60 bytes of frame, a byte per lane, then the
// stream's bytes, 64 at a time.  Every byte lies inside [roff[i], roff[i + 1]).
__global__ __launch_bounds__(64) void k_rec_write(const uint8_t* __restrict__ sig, const uint64_t* __restrict__ seq,
                                                  uint64_t n, const uint8_t* __restrict__ stream,
                                                  const uint64_t* __restrict__ soff,
                                                  const uint64_t* __restrict__ roff, uint8_t* out)
{
	const uint32_t j = threadIdx.x;
	for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
		const uint64_t sq = seq[i], a = soff[i], sl = soff[i + 1] - a;
		uint8_t* o = out + roff[i];
		const uint32_t frame = sq == kDbSeqDeleted ? 56 : 60;
		if (j < frame) {
			uint32_t v;
			if (j < 4) {
				v = kDbRecMagic >> (8 * j);
			} else if (j < 8) {
				v = 40u >> (8 * (j - 4));
			} else if (j < 48) {
				const uint32_t nib = (sig[20 * i + ((j - 8) >> 1)] >> (j & 1 ? 0 : 4)) & 15;
				v = nib < 10 ? '0' + nib : 'a' + (nib - 10);
			} else if (j < 56) {
				v = (uint32_t)(sq >> (8 * (j - 48)));
			} else {
				v = (uint32_t)sl >> (8 * (j - 56));
			}
			o[j] = (uint8_t)v;
		}
		if (frame == 60)
			for (uint64_t k = j; k < sl; k += 64)
				o[60 + k] = stream[a + k];
	}
}

}  // namespace syz

extern "C" int syzsig_deflate_dev(syzsig_ctx* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                                  const uint32_t* d_src_len, uint64_t n, uint8_t* d_out, uint64_t out_cap,
                                  uint64_t* d_out_off, uint64_t* out_bytes)
{
	SYZ_LOCK(ctx);
	if (out_bytes)
		*out_bytes = 0;
	SYZ_DB_ARGS(deflate_args(ctx, d_src, nbytes, d_src_off, d_src_len, n, d_out, out_cap, d_out_off, out_bytes));
	std::fill(ctx->df_stats, ctx->df_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	if (n == 0) {
		SYZ_HIP(hipMemsetAsync(d_out_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const uint64_t list_cap = std::min<uint64_t>(n, nbytes / (kDefLong + 1)) + 1;
	uint32_t* list;
	char* meta;  // olen[n], then ooff[n + 1], held back until the call's end
	const size_t o_off = align256(n * 4);
	SYZ_TRY(ws_get(ctx, kWsInfList, list_cap * 4, (void**)&list));
	SYZ_TRY(ws_get(ctx, kWsInfMeta, o_off + (n + 1) * 8, (void**)&meta));
	uint32_t* olen = (uint32_t*)meta;
	uint64_t* ooff = (uint64_t*)(meta + o_off);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_def_prep<<<grid_for(n, 256), 256, 0, s>>>(d_src_off, d_src_len, n, nbytes, list, list_cap, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_DB_ARGS(deflate_ranges_status(ctx->h_cnt[kCntError], ctx->h_cnt[kIfDynamic]));
	const uint64_t nlong = ctx->h_cnt[kIfLong];
	if (nlong >= list_cap)
		return fail(SYZSIG_EIO, "deflate: internal: more long values than nbytes holds");
	const unsigned waves = (unsigned)((n + 63) / 64), lwaves = (unsigned)((nlong + 63) / 64);
	k_def_wave<false><<<waves, 64, 0, s>>>(d_src, d_src_off, d_src_len, n, olen, nullptr, nullptr, ctx->d_cnt);
	if (nlong)
		k_def_long<false><<<lwaves, 64, 0, s>>>(d_src, d_src_off, d_src_len, list, nlong, olen, nullptr, nullptr,
		                                       ctx->d_cnt);
	k_inf_scan<uint32_t><<<1, 256, 0, s>>>(olen, n, ooff);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, ooff + n, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	*out_bytes = total;
	ctx->df_stats[0] = ctx->h_cnt[kIfShort];
	ctx->df_stats[1] = nlong;
	ctx->df_stats[2] = ctx->h_cnt[kIfStored];
	ctx->df_stats[3] = ctx->h_cnt[kIfFixed];
	SYZ_DB_ARGS(write_room(total, out_cap, d_out == nullptr, "deflate: the output is longer than out_cap"));
	if (d_out && total) {
		k_def_wave<true><<<waves, 64, 0, s>>>(d_src, d_src_off, d_src_len, n, olen, ooff, d_out, ctx->d_cnt);
		if (nlong)
			k_def_long<true><<<lwaves, 64, 0, s>>>(d_src, d_src_off, d_src_len, list, nlong, olen, ooff, d_out,
			                                      ctx->d_cnt);
		SYZ_HIP(hipGetLastError());
	}
	SYZ_HIP(hipMemcpyAsync(d_out_off, ooff, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_deflate_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::df_stats, out, "deflate_stats");
}

extern "C" int syzsig_deflate_host(const uint8_t* src, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len)
{
	if (out_len)
		*out_len = 0;
	SYZ_DB_ARGS(deflate_host_args(src, len, out, cap, out_len, SYZSIG_INFLATE_MAX_OUT));
	DeflateTabArray t;
	const DeflateResult r = deflate_stream(src, len, nullptr, 0, 0, t);
	*out_len = r.out_len;
	SYZ_DB_ARGS(write_room(r.out_len, cap, out == nullptr, "deflate_host: the stream is longer than cap"));
	if (out && r.out_len)
		(void)deflate_stream(src, len, out, r.out_len, r.out_len, t);
	return SYZSIG_OK;
}

extern "C" int syzsig_db_records_dev(syzsig_ctx* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n,
                                     const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_stream_off,
                                     uint8_t* d_out, uint64_t out_cap, uint64_t* d_rec_off, uint64_t* out_bytes)
{
	SYZ_LOCK(ctx);
	if (out_bytes)
		*out_bytes = 0;
	SYZ_DB_ARGS(db_records_args(ctx, d_sig, d_seq, n, d_stream, stream_bytes, d_stream_off, d_out, out_cap, d_rec_off,
	                            out_bytes));
	const hipStream_t s = ctx->stream;
	if (n == 0) {
		SYZ_HIP(hipMemsetAsync(d_rec_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	char* meta;  // rlen[n], then roff[n + 1], held back until the call's end
	const size_t o_off = align256(n * 8);
	SYZ_TRY(ws_get(ctx, kWsInfMeta, o_off + (n + 1) * 8, (void**)&meta));
	uint64_t* rlen = (uint64_t*)meta;
	uint64_t* roff = (uint64_t*)(meta + o_off);
	SYZ_TRY(counters_reset(ctx));
	k_rec_len<<<grid_for(n, 256), 256, 0, s>>>(d_seq, d_stream_off, n, stream_bytes, rlen, ctx->d_cnt);
	k_inf_scan<uint64_t><<<1, 256, 0, s>>>(rlen, n, roff);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, roff + n, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	SYZ_DB_ARGS(db_records_status(ctx->h_cnt[kCntError], ctx->h_cnt[kCntAux], ctx->h_cnt[kCntTouched]));
	*out_bytes = total;
	SYZ_DB_ARGS(write_room(total, out_cap, d_out == nullptr, "db_records: the output is longer than out_cap"));
	if (d_out)
		k_rec_write<<<grid_cap(n, 1u << 16), 64, 0, s>>>(d_sig, d_seq, n, d_stream, d_stream_off, roff, d_out);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipMemcpyAsync(d_rec_off, roff, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}
