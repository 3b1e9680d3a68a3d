/*
 * pc_sample: a program-counter sampler for a host without perf.
 *
 * A SIGALRM handler on ITIMER_REAL records, for every tick that lands on
 * the thread that started it, the interrupted program counter and, where
 * that lies outside the address range of interest, the first of the top
 * stack words that points into the range: the return address into it of
 * a shallow call out of it (the interpreter, libc, the vdso).  Samples go
 * into a buffer allocated before the timer starts; the handler allocates
 * nothing and calls nothing but pthread_self.
 *
 * Loaded with ctypes by tools/pc_sample.py.  x86-64 and aarch64 Linux.
 */

#define _GNU_SOURCE
#include <pthread.h>
#include <signal.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <ucontext.h>

#define STACK_WORDS 56

static uint64_t *g_pc, *g_via;
static volatile long g_n;
static long g_cap;
static long g_missed;           /* ticks on other threads or past the cap */
static uintptr_t g_lo, g_hi;
static pthread_t g_thread;
static struct sigaction g_old;
static int g_on;

static void
on_tick(int sig, siginfo_t *info, void *uc_)
{
    ucontext_t *uc = (ucontext_t *)uc_;
    (void)sig; (void)info;
    if (!pthread_equal(pthread_self(), g_thread) || g_n >= g_cap) {
        g_missed++;
        return;
    }
#if defined(__x86_64__)
    uintptr_t pc = (uintptr_t)uc->uc_mcontext.gregs[REG_RIP];
    uintptr_t sp = (uintptr_t)uc->uc_mcontext.gregs[REG_RSP];
#elif defined(__aarch64__)
    uintptr_t pc = (uintptr_t)uc->uc_mcontext.pc;
    uintptr_t sp = (uintptr_t)uc->uc_mcontext.sp;
#else
#error "pc_sample: x86-64 or aarch64"
#endif
    uintptr_t via = 0;
    if (pc < g_lo || pc >= g_hi) {
        /* the stack grows down: the words above sp are the frames of the
         * callers, mapped up to the thread's stack base, which on the
         * sampled thread lies far beyond these few */
        const uintptr_t *w = (const uintptr_t *)(sp & ~(uintptr_t)7);
        for (int i = 0; i < STACK_WORDS; i++) {
            if (w[i] >= g_lo && w[i] < g_hi) {
                via = w[i];
                break;
            }
        }
    }
    long n = g_n;
    g_pc[n] = pc;
    g_via[n] = via;
    g_n = n + 1;
}

/* Sample the calling thread at `hz` into room for `cap` samples; [lo, hi)
 * is the address range of interest.  0, or -1 on failure. */
int
pcs_start(int hz, uint64_t lo, uint64_t hi, long cap)
{
    if (g_on || hz <= 0 || cap <= 0)
        return -1;
    g_pc = (uint64_t *)calloc((size_t)cap, sizeof(uint64_t));
    g_via = (uint64_t *)calloc((size_t)cap, sizeof(uint64_t));
    if (g_pc == NULL || g_via == NULL)
        return -1;
    g_cap = cap;
    g_n = 0;
    g_missed = 0;
    g_lo = (uintptr_t)lo;
    g_hi = (uintptr_t)hi;
    g_thread = pthread_self();
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = on_tick;
    sa.sa_flags = SA_SIGINFO | SA_RESTART;
    sigemptyset(&sa.sa_mask);
    if (sigaction(SIGALRM, &sa, &g_old) < 0)
        return -1;
    struct itimerval it;
    it.it_interval.tv_sec = 0;
    it.it_interval.tv_usec = 1000000 / hz;
    it.it_value = it.it_interval;
    if (setitimer(ITIMER_REAL, &it, NULL) < 0) {
        sigaction(SIGALRM, &g_old, NULL);
        return -1;
    }
    g_on = 1;
    return 0;
}

/* Stop the timer and put the old handler back; the number of samples. */
long
pcs_stop(void)
{
    if (!g_on)
        return g_n;
    struct itimerval it;
    memset(&it, 0, sizeof(it));
    setitimer(ITIMER_REAL, &it, NULL);
    /* a last tick may still be on its way: where the old disposition was
     * the default one, which ends the process, ignore it instead */
    if (!(g_old.sa_flags & SA_SIGINFO) && g_old.sa_handler == SIG_DFL)
        g_old.sa_handler = SIG_IGN;
    sigaction(SIGALRM, &g_old, NULL);
    g_on = 0;
    return g_n;
}

long pcs_missed(void) { return g_missed; }
const uint64_t *pcs_pcs(void) { return g_pc; }
const uint64_t *pcs_vias(void) { return g_via; }

void
pcs_free(void)
{
    if (g_on)
        return;
    free(g_pc);
    free(g_via);
    g_pc = g_via = NULL;
    g_n = g_cap = 0;
}
