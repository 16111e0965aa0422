// ref_harness.cc -- drives the REFERENCE executor's own per-call output code on
// synthetic KCOV buffers to produce golden vectors.  TEST INFRASTRUCTURE ONLY.
//
// Built by oracle/Makefile (container only, needs /root/reference) into
// oracle/_ref/ref_harness.  It #includes the reference translation unit
// executor/executor_linux.cc unchanged (its main renamed), so every function that
// runs here -- handle_completion (executor.h:530-608), write_coverage_signal<uint64>
// (:492-528, the cover output :514-527 included), hash/dedup (:677-706),
// kcov_comparison_t::write and its operators (:823-875), read_cover_size /
// cover_check / write_output / write_completed / kcov_comparison_t::ignore
// (executor_linux.cc:179-253) -- is the reference's own code, compiled with the
// reference Makefile's flags (Makefile:139-143).  No reference source is copied.
//
// Protocol (little-endian, stdin):
//   u32 magic (kProtocol: a binary built from an older version of this file refuses the
//   input, and its output lacks the word, so a stale build is noticed and not believed),
//   u32 mode (0 signal, 1 cover, 2 comps), u32 flags (bit 0: flag_dedup_cover),
//   u64 out_addr (where to map the output region; 0: anywhere), u32 nprog;
//   per program: u32 ncalls; per call: u32 failed (errno != 0), u32 n, then
//     modes 0 and 1: u64 pc[n]
//     mode 2:        u64 rec[n][4] = (type, arg1, arg2, pc), as KCOV_TRACE_CMP lays
//                    them out after the count word
// Output (stdout): u32 magic (kProtocol), u64 output_data (the address ignore() compares operands with);
//   per program: u32 status (the child's exit status; 0x100 | signal if it was
//   killed), u32 nwords, then the executor's output region words [0, nwords):
//   word 0 = completed count (write_completed), then per completed call the
//   record: callIndex, callNum, errno, faultInjected, nsig, ncover, ncomps,
//   sig[nsig], cover[ncover], ncomps comparison records of 3 or 5 words
//   (executor.h:566-604).
// Modes set the executor's flags and nothing else:
//   signal: flag_collect_cover = flag_collect_comps = false
//   cover:  flag_collect_cover = true, flag_dedup_cover from the input
//   comps:  flag_collect_comps = true
// th->cover_end is what cover_open sets (executor_linux.cc:146-149): cover_data +
// kCoverSize * 8, so the reference's own fail("too many comparisons") decides how
// many records a call may hold; the buffer behind it is larger.
// Each program runs in a forked child, exactly like the executor's per-program
// fork (common_linux.h:1995-2030): the dedup table starts zeroed, a cover_check
// failure's doexit(0) and a fail()'s doexit(kFailStatus) end only that child.
#define main syz_reference_executor_main
#include "executor_linux.cc"
#undef main

#include <sys/mman.h>
#include <vector>

#ifndef MAP_FIXED_NOREPLACE
#define MAP_FIXED_NOREPLACE 0x100000
#endif

const uint32 kProtocol = 0x32485a53; // "SZH2"

enum { MODE_SIGNAL = 0,
       MODE_COVER = 1,
       MODE_COMPS = 2 };

static bool read_exact(void* p, size_t n)
{
	char* c = (char*)p;
	while (n) {
		ssize_t r = read(0, c, n);
		if (r <= 0)
			return false;
		c += r;
		n -= r;
	}
	return true;
}

static void write_exact(const void* p, size_t n)
{
	const char* c = (const char*)p;
	while (n) {
		ssize_t r = write(1, c, n);
		if (r <= 0)
			doexit(2);
		c += r;
		n -= r;
	}
}

struct call_in {
	uint32 failed;
	uint32 n;
	std::vector<uint64> words;
};

int main()
{
	uint32 magic = 0, hdr0[2];
	uint64 out_addr = 0;
	uint32 nprog = 0;
	if (!read_exact(&magic, 4) || magic != kProtocol)
		return 5;
	if (!read_exact(hdr0, 8) || !read_exact(&out_addr, 8) || !read_exact(&nprog, 4))
		return 1;
	const uint32 mode = hdr0[0];
	if (mode > MODE_COMPS)
		return 1;
	const size_t per = mode == MODE_COMPS ? 4 : 1; // u64 words per entry
	// Shared output region (kMaxOutput, executor.h:24), like the executor's shmem out file
	// (executor_linux.cc:61-65 maps it at a chosen address too).
	uint32* shared = (uint32*)mmap((void*)out_addr, kMaxOutput, PROT_READ | PROT_WRITE,
				       MAP_SHARED | MAP_ANONYMOUS | (out_addr ? MAP_FIXED_NOREPLACE : 0), -1, 0);
	if (shared == MAP_FAILED || (out_addr && (uint64)shared != out_addr))
		return 4;
	// Per-thread KCOV-like buffer: word 0 = count, then the PCs or the comparison records
	// (executor_linux.cc:143-149).  Twice the executor's, so that a call past its limit
	// still fits and the executor's own check is what refuses it.
	const size_t cover_words = 2 * (size_t)kCoverSize + 1;
	uint64* cover = (uint64*)mmap(0, cover_words * sizeof(uint64), PROT_READ | PROT_WRITE,
				      MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
	if (cover == MAP_FAILED)
		return 1;
	uint64 addr = (uint64)shared;
	write_exact(&kProtocol, 4);
	write_exact(&addr, 8);
	for (uint32 p = 0; p < nprog; p++) {
		uint32 ncalls = 0;
		if (!read_exact(&ncalls, 4))
			return 1;
		std::vector<call_in> calls(ncalls);
		for (uint32 c = 0; c < ncalls; c++) {
			uint32 hdr[2];
			if (!read_exact(hdr, 8))
				return 1;
			calls[c].failed = hdr[0];
			calls[c].n = hdr[1];
			if (1 + per * (size_t)hdr[1] > cover_words)
				return 1;
			calls[c].words.resize(per * (size_t)hdr[1]);
			if (hdr[1] && !read_exact(calls[c].words.data(), 8 * calls[c].words.size()))
				return 1;
		}
		memset(shared, 0, 4096);
		pid_t pid = fork();
		if (pid < 0)
			return 1;
		if (pid == 0) {
			// Child == one executor worker executing one program.
			is_kernel_64_bit = true;
			flag_cover = true;
			flag_collect_cover = mode == MODE_COVER;
			flag_dedup_cover = (hdr0[1] & 1) != 0;
			flag_collect_comps = mode == MODE_COMPS;
			collide = false;
			output_data = shared;
			output_pos = output_data; // common_linux.h:2026
			write_output(0); // executor.h:297, number of executed syscalls
			thread_t* th = &threads[0];
			th->cover_data = (char*)cover;
			if (mode == MODE_SIGNAL)
				th->cover_end = (char*)(cover + kCoverSize + 1);
			else
				th->cover_end = th->cover_data + (size_t)kCoverSize * 8; // executor_linux.cc:146-149
			for (uint32 c = 0; c < ncalls; c++) {
				event_init(&th->ready);
				event_init(&th->done);
				event_set(&th->done);
				th->handled = false;
				th->colliding = false;
				th->call_index = c;
				th->call_num = c;
				th->copyout_index = no_copyout;
				th->res = calls[c].failed ? -1 : 0;
				th->reserrno = calls[c].failed ? EINVAL : 0;
				th->fault_injected = false;
				// A successful call reads copyout instructions; give it instr_eof.
				*(uint64*)input_data = instr_eof;
				th->copyout_pos = (uint64*)input_data;
				cover[0] = calls[c].n;
				memcpy(cover + 1, calls[c].words.data(), 8 * calls[c].words.size());
				th->cover_size = read_cover_size(th); // executor_linux.cc:179-189
				running = 1;
				handle_completion(th);
			}
			doexit(0);
		}
		int status = 0;
		if (waitpid(pid, &status, 0) != pid)
			return 1;
		uint32 st = WIFEXITED(status) ? (uint32)WEXITSTATUS(status) : 0x100u | (uint32)WTERMSIG(status);
		// Walk the records to find the used length.
		uint32 completed = shared[0];
		size_t pos = 1;
		const size_t limit = kMaxOutput / 4;
		for (uint32 r = 0; r < completed; r++) {
			if (pos + 7 > limit)
				return 3;
			uint32 nsig = shared[pos + 4], ncover = shared[pos + 5], ncomps = shared[pos + 6];
			pos += 7 + (size_t)nsig + ncover;
			for (uint32 k = 0; k < ncomps; k++) {
				if (pos >= limit)
					return 3;
				// executor.h:848-858: a record is its type word and two operands of one or two words
				pos += (shared[pos] & KCOV_CMP_SIZE_MASK) == KCOV_CMP_SIZE8 ? 5 : 3;
			}
			if (pos > limit)
				return 3;
		}
		uint32 nwords = (uint32)pos;
		write_exact(&st, 4);
		write_exact(&nwords, 4);
		write_exact(shared, 4 * pos);
	}
	return 0;
}
