// db.hip -- pkg/db's read side: the frames of a database file on the host
// (syzsig_db_scan) and its values through a batched RFC 1951 decoder on the
// device (syzsig_inflate_dev).  The map's last-write-wins, syzsig_db_live_dev, is
// the third client of the Sig sets' sort and lives next to it in sigs.hip.
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
__global__ __launch_bounds__(256) void k_inf_scan(const uint32_t* __restrict__ olen, uint64_t n, uint64_t* ooff)
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
	k_inf_scan<<<1, 256, 0, s>>>(olen, n, ooff);
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
