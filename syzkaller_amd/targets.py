"""The KCOV target of Device.edge_derive / Device.edge_cover: which of the
reference executor's write_coverage_signal<cover_t> instantiations and which of
its cover_check bodies a kernel's traces go through (include/syzsig.h
SYZSIG_TARGET_*).

The reference picks cover_t at run time (executor/executor.h:595-598:
is_kernel_64_bit ? uint64 : uint32) and cover_check at build time:
  - is_kernel_64_bit starts true (executor.h:71) and only the Linux executor
    ever changes it (executor_linux.cc:46, detect_kernel_bitness :255-275: true
    where sizeof(void*) == 8, else the width of /proc/kallsyms addresses), then
    asks the kernel for KCOV_INIT_TRACE32 (:143-146);
  - cover_check(uint32) is `return true` in every executor;
  - cover_check(uint64) is the x86 text range only in a Linux executor built
    for i386 or x86_64 (executor_linux.cc:196-204), `return true` otherwise.
"""
from ._lib import SYZSIG_TARGET_CHECK_X86, SYZSIG_TARGET_LINUX_AMD64, SYZSIG_TARGET_PC32

__all__ = ["PC32", "CHECK_X86", "LINUX_AMD64", "for_kernel", "is_valid"]

PC32 = SYZSIG_TARGET_PC32
CHECK_X86 = SYZSIG_TARGET_CHECK_X86
LINUX_AMD64 = SYZSIG_TARGET_LINUX_AMD64

# (os, arch) -> (target on a 64-bit kernel, target on a 32-bit kernel or None where the reference has none)
_TABLE = {
    # executor_linux.cc:196-204, the __x86_64__ branch; sizeof(void*) == 8 (:257-258)
    ("linux", "amd64"): (CHECK_X86, None),
    # the __i386__ branch of :198 when kallsyms is wide (:264-274), else uint32 (executor.h:595-598) and :191-194
    ("linux", "386"): (CHECK_X86, PC32),
    # a 32-bit executor on the 32-bit kernels this reference targets: uint32, executor_linux.cc:191-194
    ("linux", "arm"): (PC32, PC32),
    # sizeof(void*) == 8, and the #else of executor_linux.cc:201-202
    ("linux", "arm64"): (0, None),
    ("linux", "ppc64le"): (0, None),
    # executor_bsd.cc:166 (is_kernel_64_bit never changes), :228-231 `return true`
    ("freebsd", "amd64"): (0, None),
    ("netbsd", "amd64"): (0, None),
    # executor_fuchsia.cc:64-67
    ("fuchsia", "amd64"): (0, None),
    # executor_akaros.cc:104-107
    ("akaros", "amd64"): (0, None),
    # executor_windows.cc:67-70
    ("windows", "amd64"): (0, None),
}


def is_valid(target):
    """0, PC32 or CHECK_X86: the reference has no executor with a checked u32 PC."""
    return target in (0, PC32, CHECK_X86)


def for_kernel(os, arch, kernel_64_bit=True):
    """The target of the kernel under test: `os` / `arch` as syzkaller names them
    (mgrconfig's target "linux/amd64" split at the slash), kernel_64_bit what the
    executor's detect_kernel_bitness finds (it matters for linux/386 alone, the
    one 32-bit executor that runs on either kernel)."""
    try:
        wide, narrow = _TABLE[(os, arch)]
    except KeyError:
        raise ValueError(f"no KCOV target known for {os}/{arch}") from None
    if kernel_64_bit:
        return wide
    if narrow is None:
        raise ValueError(f"{os}/{arch} has no 32-bit kernel in the reference")
    return narrow
