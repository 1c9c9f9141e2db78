// host_kernel.hpp — how the host code launches a kernel: launch() takes the kernel itself and converts every argument to the type the kernel declares for it,
// with_flag() / with_flags() turn run-time bools into template arguments.  Part of the single translation unit idkpt.hip (included there, before the host_*.hpp files).
#pragma once
#include <type_traits>

template <class T> struct kernel_arg { using type = T; };   // (a non-deduced context: the parameter types come from the kernel's signature alone)

// launch(k_name<ARGS>, grid, block, ldsBytes, stream, args...): an argument of the wrong type, one too few or one too many is a compile error; nullptr, non-const
// pointers and DevBuf::as<T>() convert as in a plain call.  Arguments already of the kernel's type are passed on by reference (DScene and Frame are not copied twice).
template <class... P>
static inline __attribute__((always_inline)) void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t ldsBytes, hipStream_t st, const typename kernel_arg<P>::type&... args)
{
    hipLaunchKernelGGL(kernel, grid, block, ldsBytes, st, args...);
}

// with_flag(b, [&](auto B) { launch(k_name<B>, ...); }): the launch is written once, B is std::true_type or std::false_type.  Every combination the lambda is called
// with is instantiated, so where only some combinations of two flags exist the `if` that says so stays at the call site.
template <int N> using int_c = std::integral_constant<int, N>;   // (the same for the developer build's probes, whose run-time choice is a number)
template <class F> static inline void with_flag(bool a, F&& f) { if (a) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static inline void with_flags(bool a, bool b, F&& f) { with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); }); }
