/*
 * cueball_amd._speed: native event/FSM runtime core.
 *
 * The framework's hot loop (a pool claim/release cycle) walks six-plus
 * Moore-machine state transitions across three FSMs, each with scoped
 * listener registration/teardown and async stateChanged queueing (see
 * cueball_amd/fsm.py for the semantics contract, which this module
 * reproduces exactly -- the whole pytest suite runs against either
 * implementation).  This C++ core removes the interpreter overhead from
 * EventEmitter dispatch, scope bookkeeping and the transition loop.
 *
 * The reference (node-cueball) has no native code; this is the one
 * component where a native core is justified by measurement (see
 * profiles/README.md): event-loop throughput is the library's
 * performance story.
 *
 * Plain C++/CPython API -- no GPU code exists in this problem domain
 * (SURVEY.md section 0).
 */

#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <structmember.h>
#include <cmath>
#include <cstring>
#include <ctime>

#include "lathist.h"

/* The library's own listeners of the claim cycle are intrinsic hooks of
 * the core (profiles/claim_cycle_intrinsic.md).  Each part can be
 * switched back on its own at build time, e.g.
 * CFLAGS=-DCUEBALL_HANDLE_HOOKS=0, for the leave-one-out measurements:
 *   CUEBALL_HANDLE_HOOKS  the ticket and the busy slot's reaction to
 *                         released/closed are fields of the handle
 *   CUEBALL_SLOT_HOOKS    the slot kit's smgr/unwanted listeners of the
 *                         busy and idle states are hooks of the emission
 *   CUEBALL_LAZY_SCOPES   a transition's scope is made when first asked for
 *   CUEBALL_VECTORCALL    the core's own callables take vectorcall, and
 *                         ConnectionPool.claim has a native entry
 * Per-claim lookups whose answer is the same on every claim
 * (profiles/claim_cycle_lookups.md):
 *   CUEBALL_LEAK_TAG      the leak detector's cached counts are confirmed
 *                         by the event table's version, not by four lookups
 *   CUEBALL_OWN_CONN_ERR  the claimed handle registers and removes its
 *                         connection-error listener itself, without a scope */
#ifndef CUEBALL_LEAK_TAG
#define CUEBALL_LEAK_TAG 1
#endif
#ifndef CUEBALL_OWN_CONN_ERR
#define CUEBALL_OWN_CONN_ERR 1
#endif
/* dicts carry a version that moves on every change of the dict itself
 * (not of its values' contents) up to CPython 3.11; later versions keep
 * the four lookups */
#if CUEBALL_LEAK_TAG && PY_VERSION_HEX >= 0x030C0000
#undef CUEBALL_LEAK_TAG
#define CUEBALL_LEAK_TAG 0
#endif
#ifndef CUEBALL_HANDLE_HOOKS
#define CUEBALL_HANDLE_HOOKS 1
#endif
#ifndef CUEBALL_SLOT_HOOKS
#define CUEBALL_SLOT_HOOKS 1
#endif
#ifndef CUEBALL_LAZY_SCOPES
#define CUEBALL_LAZY_SCOPES 1
#endif
#ifndef CUEBALL_VECTORCALL
#define CUEBALL_VECTORCALL 1
#endif
#ifndef CUEBALL_EXACT_TYPES
#define CUEBALL_EXACT_TYPES 1
#endif
#ifndef CUEBALL_VALID_IDENTITY
#define CUEBALL_VALID_IDENTITY 1
#endif
#if !defined(Py_TPFLAGS_HAVE_VECTORCALL) && defined(_Py_TPFLAGS_HAVE_VECTORCALL)
#define Py_TPFLAGS_HAVE_VECTORCALL _Py_TPFLAGS_HAVE_VECTORCALL
#endif

namespace {

/* interned strings, created at module init */
PyObject *s_stateChanged;
PyObject *s_listener;
PyObject *s_on;
PyObject *s_remove_listener;
PyObject *s_call_soon;
PyObject *s_call_later;
PyObject *s_cancel;
PyObject *s_state_prefix;      /* "state_" */
PyObject *s_dot;               /* "." */
PyObject *s_underscore;        /* "_" */
PyObject *s_flush_name;        /* "_flush_state_changed" */
PyObject *s_internal;          /* "_cueball_internal" */
PyObject *s_is_closed;         /* "is_closed" */

PyObject *g_get_loop;          /* python helper: get_loop(loop) */
PyObject *g_fsm_error;         /* exception class FSMError */
PyObject *g_entry_name_cache;  /* dict: state name -> "state_x_y" */
PyObject *g_flush_batches;     /* dict: loop -> _FlushBatch */
PyObject *g_tracer;            /* optional fn(fsm, state) on transitions */
PyObject *g_remove_desc;       /* EmitterType's remove_listener descriptor */

/* get_loop(loop): a loop that is given is the answer; only None needs
 * the python helper (running loop, else the policy's).  New reference. */
static inline PyObject *
resolve_loop(PyObject *loop)
{
    if (loop != NULL && loop != Py_None) {
        Py_INCREF(loop);
        return loop;
    }
    return PyObject_CallOneArg(g_get_loop, Py_None);
}

/* ------------------------------------------------------------------ */
/* EventEmitter                                                        */
/* ------------------------------------------------------------------ */

typedef struct {
    PyObject_HEAD
    PyObject *ev_events;   /* dict: str -> list of callables; a list that
                            * has been emptied stays (see
                            * Emitter_remove_listener) */
    PyObject *ev_dict;     /* instance __dict__ (lazy) */
    PyObject *ev_weakrefs;
    /* leak-detector cache (see emitter_leak_counts): ev_gen moves on
     * every add/remove of a listener the detector could count */
    unsigned long ev_gen;
    struct LeakCache *ev_lk;    /* NULL until the detector first counts:
                                 * only claimed connections have one, so
                                 * the other emitters (every claim handle
                                 * is one) do not carry its fields */
} Emitter;

struct LeakCache {
    int lk_ok;
    unsigned long lk_gen;       /* ev_gen the cache was filled at */
    long lk_cnt[4];             /* counted listeners per leak event */
    Py_ssize_t lk_len[4];       /* list lengths the counts belong to */
    uint64_t lk_ver;            /* ev_events' version it was filled at */
    PyObject *lk_list[4];       /* the lists the lengths were read from,
                                 * owned, NULL where the table had none */
};

extern PyTypeObject EmitterType;
extern PyTypeObject ConnErrCbType;
extern PyTypeObject KitCbType;

/* This module's own callback types answer _cueball_internal as true and
 * are never counted by the leak detector, so (un)registering one leaves
 * the cached counts valid. */
static inline int
listener_is_own_internal(PyObject *listener)
{
    PyTypeObject *tp = Py_TYPE(listener);
    return tp == &ConnErrCbType || tp == &KitCbType;
}

/* Listener lists on the claim cycle go 0 -> 1 -> 0 entries every cycle.
 * list.append / slice deletion give the item array back to the
 * allocator at 0 and fetch it again at 1; these two keep a small array
 * in place. */
#define SMALL_LIST_KEEP 8

static inline int
list_append_keep(PyObject *ls, PyObject *item)
{
    PyListObject *l = (PyListObject *)ls;
    Py_ssize_t n = Py_SIZE(l);
    if (n < l->allocated) {
        Py_INCREF(item);
        l->ob_item[n] = item;
        Py_SET_SIZE(l, n + 1);
        return 0;
    }
    return PyList_Append(ls, item);
}

static inline int
list_remove_at_keep(PyObject *ls, Py_ssize_t i)
{
    PyListObject *l = (PyListObject *)ls;
    Py_ssize_t n = Py_SIZE(l);
    if (l->allocated > SMALL_LIST_KEEP)
        return PyList_SetSlice(ls, i, i + 1, NULL);
    PyObject *item = l->ob_item[i];
    for (Py_ssize_t j = i; j + 1 < n; j++)
        l->ob_item[j] = l->ob_item[j + 1];
    Py_SET_SIZE(l, n - 1);
    Py_DECREF(item);
    return 0;
}

int
Emitter_init(PyObject *self_, PyObject *args, PyObject *kwds)
{
    Emitter *self = (Emitter *)self_;
    (void)args; (void)kwds;
    if (self->ev_events == NULL) {
        self->ev_events = PyDict_New();
        if (self->ev_events == NULL)
            return -1;
    }
    return 0;
}

int
Emitter_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Emitter *self = (Emitter *)self_;
    Py_VISIT(self->ev_events);
    Py_VISIT(self->ev_dict);
    if (self->ev_lk != NULL)
        for (int i = 0; i < 4; i++)
            Py_VISIT(self->ev_lk->lk_list[i]);
    return 0;
}

/* forget the leak detector's cached counts and the lists they hold */
static void
emitter_lk_drop(Emitter *self)
{
    LeakCache *lk = self->ev_lk;
    if (lk == NULL)
        return;
    lk->lk_ok = 0;
    for (int i = 0; i < 4; i++)
        Py_CLEAR(lk->lk_list[i]);
}

int
Emitter_clear_(PyObject *self_)
{
    Emitter *self = (Emitter *)self_;
    LeakCache *lk = self->ev_lk;
    if (lk != NULL) {
        self->ev_lk = NULL;
        for (int i = 0; i < 4; i++)
            Py_CLEAR(lk->lk_list[i]);
        PyMem_Free(lk);
    }
    Py_CLEAR(self->ev_events);
    Py_CLEAR(self->ev_dict);
    return 0;
}

void
Emitter_dealloc(PyObject *self_)
{
    Emitter *self = (Emitter *)self_;
    PyTypeObject *tp = Py_TYPE(self_);
    PyObject_GC_UnTrack(self_);
    if (self->ev_weakrefs != NULL)
        PyObject_ClearWeakRefs(self_);
    Emitter_clear_(self_);
    tp->tp_free(self_);
}

/* core: register a listener */
PyObject *
emitter_add(Emitter *self, PyObject *event, PyObject *listener)
{
    if (self->ev_events == NULL) {
        self->ev_events = PyDict_New();
        if (self->ev_events == NULL)
            return NULL;
    }
    PyObject *ls = PyDict_GetItemWithError(self->ev_events, event);
    if (ls == NULL) {
        if (PyErr_Occurred())
            return NULL;
        ls = PyList_New(0);
        if (ls == NULL)
            return NULL;
        if (PyDict_SetItem(self->ev_events, event, ls) < 0) {
            Py_DECREF(ls);
            return NULL;
        }
        Py_DECREF(ls);  /* dict holds it */
    }
    if (list_append_keep(ls, listener) < 0)
        return NULL;
    if (!listener_is_own_internal(listener))
        self->ev_gen++;
    Py_INCREF(listener);
    return listener;
}

PyObject *
Emitter_on(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "on(event, listener)");
        return NULL;
    }
    return emitter_add((Emitter *)self_, args[0], args[1]);
}

/* once() wrapper object */
typedef struct {
    PyObject_HEAD
    PyObject *ow_emitter;   /* weak semantics not needed; strong ref */
    PyObject *ow_event;
    PyObject *ow_listener;
} OnceWrapper;

extern PyTypeObject OnceWrapperType;

PyObject *
OnceWrapper_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    OnceWrapper *self = (OnceWrapper *)self_;
    (void)kwds;
    /* remove ourselves first (reference events.py once semantics) */
    PyObject *res = PyObject_CallMethodObjArgs(
        self->ow_emitter, s_remove_listener, self->ow_event,
        (PyObject *)self, NULL);
    if (res == NULL)
        return NULL;
    Py_DECREF(res);
    return PyObject_Call(self->ow_listener, args, NULL);
}

PyObject *
OnceWrapper_get_listener(PyObject *self_, void *closure)
{
    OnceWrapper *self = (OnceWrapper *)self_;
    (void)closure;
    Py_INCREF(self->ow_listener);
    return self->ow_listener;
}

int
OnceWrapper_traverse(PyObject *self_, visitproc visit, void *arg)
{
    OnceWrapper *self = (OnceWrapper *)self_;
    Py_VISIT(self->ow_emitter);
    Py_VISIT(self->ow_event);
    Py_VISIT(self->ow_listener);
    return 0;
}

int
OnceWrapper_clear_(PyObject *self_)
{
    OnceWrapper *self = (OnceWrapper *)self_;
    Py_CLEAR(self->ow_emitter);
    Py_CLEAR(self->ow_event);
    Py_CLEAR(self->ow_listener);
    return 0;
}

void
OnceWrapper_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    OnceWrapper_clear_(self_);
    PyObject_GC_Del(self_);
}

PyGetSetDef OnceWrapper_getset[] = {
    {(char *)"listener", OnceWrapper_get_listener, NULL,
     (char *)"original listener", NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject OnceWrapperType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._OnceWrapper",       /* tp_name */
    sizeof(OnceWrapper),                      /* tp_basicsize */
    0,                                        /* tp_itemsize */
    OnceWrapper_dealloc,                      /* tp_dealloc */
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    OnceWrapper_call,                         /* tp_call */
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,  /* tp_flags */
    0,                                        /* tp_doc */
    OnceWrapper_traverse,                     /* tp_traverse */
    OnceWrapper_clear_,                       /* tp_clear */
    0, 0, 0, 0, 0, 0,
    OnceWrapper_getset,                       /* tp_getset */
};

PyObject *
Emitter_once(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "once(event, listener)");
        return NULL;
    }
    OnceWrapper *w = PyObject_GC_New(OnceWrapper, &OnceWrapperType);
    if (w == NULL)
        return NULL;
    Py_INCREF(self_);
    w->ow_emitter = self_;
    Py_INCREF(args[0]);
    w->ow_event = args[0];
    Py_INCREF(args[1]);
    w->ow_listener = args[1];
    PyObject_GC_Track((PyObject *)w);
    PyObject *r = emitter_add((Emitter *)self_, args[0], (PyObject *)w);
    if (r == NULL) {
        Py_DECREF(w);
        return NULL;
    }
    Py_DECREF(r);
    return (PyObject *)w;
}

/* remove one registration; *found_at is its index before the removal,
 * or -1 if there was none */
int
emitter_remove_core(Emitter *self, PyObject *const *args,
                    Py_ssize_t *found_at)
{
    *found_at = -1;
    if (self->ev_events == NULL)
        return 0;
    PyObject *ls = PyDict_GetItemWithError(self->ev_events, args[0]);
    if (ls == NULL)
        return PyErr_Occurred() ? -1 : 0;
    Py_ssize_t n = PyList_GET_SIZE(ls);
    Py_ssize_t found = -1;
    for (Py_ssize_t i = 0; i < n; i++) {
        PyObject *item = PyList_GET_ITEM(ls, i);
        if (item == args[1]) {
            found = i;
            break;
        }
        /* bound methods are fresh objects per attribute access: fall
         * back to == (matches list.remove semantics in the Python
         * implementation) */
        int eq = PyObject_RichCompareBool(item, args[1], Py_EQ);
        if (eq < 0)
            return -1;
        if (eq) {
            found = i;
            break;
        }
    }
    if (found < 0) {
        /* allow removing a once() registration by its inner listener */
        for (Py_ssize_t i = 0; i < n; i++) {
            PyObject *w = PyList_GET_ITEM(ls, i);
            if (Py_TYPE(w) != &OnceWrapperType)
                continue;
            PyObject *inner = ((OnceWrapper *)w)->ow_listener;
            if (inner == args[1]) {
                found = i;
                break;
            }
            int eq = PyObject_RichCompareBool(inner, args[1], Py_EQ);
            if (eq < 0)
                return -1;
            if (eq) {
                found = i;
                break;
            }
        }
    }
    if (found >= 0) {
        if (!listener_is_own_internal(PyList_GET_ITEM(ls, found)))
            self->ev_gen++;
        /* an emptied list stays in ev_events: the scoped registrations
         * of the claim cycle would otherwise delete and re-create it
         * (and its key) every cycle.  Everything that reports events
         * treats an empty list as absent. */
        if (list_remove_at_keep(ls, found) < 0)
            return -1;
        *found_at = found;
    }
    return 0;
}

PyObject *
Emitter_remove_listener(PyObject *self_, PyObject *const *args,
                        Py_ssize_t nargs)
{
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "remove_listener(event, listener)");
        return NULL;
    }
    Py_ssize_t at;
    if (emitter_remove_core((Emitter *)self_, args, &at) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
Emitter_remove_all_listeners(PyObject *self_, PyObject *const *args,
                             Py_ssize_t nargs)
{
    Emitter *self = (Emitter *)self_;
    if (self->ev_events == NULL)
        Py_RETURN_NONE;
    self->ev_gen++;
    if (nargs == 0 || args[0] == Py_None) {
        PyDict_Clear(self->ev_events);
    } else {
        if (PyDict_DelItem(self->ev_events, args[0]) < 0)
            PyErr_Clear();
    }
    Py_RETURN_NONE;
}

PyObject *
Emitter_listeners(PyObject *self_, PyObject *event)
{
    Emitter *self = (Emitter *)self_;
    if (self->ev_events != NULL) {
        PyObject *ls = PyDict_GetItemWithError(self->ev_events, event);
        if (ls != NULL)
            return PyList_GetSlice(ls, 0, PyList_GET_SIZE(ls));
        if (PyErr_Occurred())
            return NULL;
    }
    return PyList_New(0);
}

PyObject *
Emitter_listener_count(PyObject *self_, PyObject *event)
{
    Emitter *self = (Emitter *)self_;
    Py_ssize_t n = 0;
    if (self->ev_events != NULL) {
        PyObject *ls = PyDict_GetItemWithError(self->ev_events, event);
        if (ls != NULL)
            n = PyList_GET_SIZE(ls);
        else if (PyErr_Occurred())
            return NULL;
    }
    return PyLong_FromSsize_t(n);
}

PyObject *
Emitter_event_names(PyObject *self_, PyObject *noargs)
{
    Emitter *self = (Emitter *)self_;
    (void)noargs;
    PyObject *names = PyList_New(0);
    if (names == NULL || self->ev_events == NULL)
        return names;
    PyObject *key, *ls;
    Py_ssize_t pos = 0;
    while (PyDict_Next(self->ev_events, &pos, &key, &ls)) {
        /* emptied lists are kept (Emitter_remove_listener) */
        if (PyList_Check(ls) && PyList_GET_SIZE(ls) == 0)
            continue;
        if (PyList_Append(names, key) < 0) {
            Py_DECREF(names);
            return NULL;
        }
    }
    return names;
}

/* emit with node snapshot semantics */
int
emitter_emit_core(Emitter *self, PyObject *event, PyObject *const *eargs,
                  Py_ssize_t neargs)
{
    if (self->ev_events == NULL)
        return 0;
    PyObject *ls = PyDict_GetItemWithError(self->ev_events, event);
    if (ls == NULL)
        return PyErr_Occurred() ? -1 : 0;
    Py_ssize_t n = PyList_GET_SIZE(ls);
    if (n == 0)
        return 0;
    if (n == 1) {
        /* copy-free fast path (snapshot still holds: a listener added
         * during the call is not invoked) */
        PyObject *cb = PyList_GET_ITEM(ls, 0);
        Py_INCREF(cb);
        PyObject *r = PyObject_Vectorcall(cb, eargs, neargs, NULL);
        Py_DECREF(cb);
        if (r == NULL)
            return -1;
        Py_DECREF(r);
        return 1;
    }
    PyObject *snap = PyList_GetSlice(ls, 0, n);
    if (snap == NULL)
        return -1;
    for (Py_ssize_t i = 0; i < n; i++) {
        PyObject *cb = PyList_GET_ITEM(snap, i);
        PyObject *r = PyObject_Vectorcall(cb, eargs, neargs, NULL);
        if (r == NULL) {
            Py_DECREF(snap);
            return -1;
        }
        Py_DECREF(r);
    }
    Py_DECREF(snap);
    return 1;
}

PyObject *
Emitter_emit(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs < 1) {
        PyErr_SetString(PyExc_TypeError, "emit(event, *args)");
        return NULL;
    }
    int r = emitter_emit_core((Emitter *)self_, args[0], args + 1,
                              nargs - 1);
    if (r < 0)
        return NULL;
    return PyBool_FromLong(r);
}

PyMethodDef Emitter_methods[] = {
    {"on", (PyCFunction)(void (*)(void))Emitter_on, METH_FASTCALL, NULL},
    {"add_listener", (PyCFunction)(void (*)(void))Emitter_on,
     METH_FASTCALL, NULL},
    {"once", (PyCFunction)(void (*)(void))Emitter_once, METH_FASTCALL,
     NULL},
    {"remove_listener",
     (PyCFunction)(void (*)(void))Emitter_remove_listener, METH_FASTCALL,
     NULL},
    {"remove_all_listeners",
     (PyCFunction)(void (*)(void))Emitter_remove_all_listeners,
     METH_FASTCALL, NULL},
    {"listeners", Emitter_listeners, METH_O, NULL},
    {"listener_count", Emitter_listener_count, METH_O, NULL},
    {"event_names", Emitter_event_names, METH_NOARGS, NULL},
    {"emit", (PyCFunction)(void (*)(void))Emitter_emit, METH_FASTCALL,
     NULL},
    {NULL, NULL, 0, NULL},
};

PyMemberDef Emitter_members[] = {
    {(char *)"_events", T_OBJECT, offsetof(Emitter, ev_events), READONLY,
     NULL},
    {NULL, 0, 0, 0, NULL},
};

PyTypeObject EmitterType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.EventEmitter",        /* tp_name */
    sizeof(Emitter),                          /* tp_basicsize */
    0,                                        /* tp_itemsize */
    Emitter_dealloc,                          /* tp_dealloc */
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE | Py_TPFLAGS_HAVE_GC,
    "node-style EventEmitter (native)",       /* tp_doc */
    Emitter_traverse,                         /* tp_traverse */
    Emitter_clear_,                           /* tp_clear */
    0,                                        /* tp_richcompare */
    offsetof(Emitter, ev_weakrefs),           /* tp_weaklistoffset */
    0, 0,
    Emitter_methods,                          /* tp_methods */
    Emitter_members,                          /* tp_members */
    0, 0, 0, 0, 0,
    offsetof(Emitter, ev_dict),               /* tp_dictoffset */
    Emitter_init,                             /* tp_init */
    0,
    PyType_GenericNew,                        /* tp_new */
};

/* ------------------------------------------------------------------ */
/* forward decls                                                       */
/* ------------------------------------------------------------------ */

typedef struct FSMOb FSMOb;
int fsm_goto_state(FSMOb *fsm, PyObject *state);

/* ------------------------------------------------------------------ */
/* StateScope                                                          */
/* ------------------------------------------------------------------ */

typedef struct {
    PyObject_HEAD
    PyObject *sc_fsm;       /* FSMOb*, strong */
    PyObject *sc_listeners; /* flat list [em, evt, cb, ...] of the
                             * registrations beyond sc_reg, or NULL */
    PyObject *sc_timers;    /* list of cancellables or NULL */
    int sc_active;
    int sc_nreg;            /* registrations held in sc_reg */
    PyObject *sc_reg[3 * 4];/* the first four (em, evt, cb), owned: the
                             * states of the claim cycle register at
                             * most two, so they allocate nothing */
} Scope;

#define SCOPE_INLINE_REGS 4

extern PyTypeObject ScopeType;

/* Freed scopes are kept for the next state that asks for one (see
 * fsm_need_scope; of the six states of a claim cycle none does, unless
 * the handle's `claimed` is entered with CUEBALL_OWN_CONN_ERR off). */
#define SCOPE_FREELIST_MAX 32
Scope *scope_freelist[SCOPE_FREELIST_MAX];
int scope_freelist_n = 0;

Scope *
scope_new(PyObject *fsm)
{
    Scope *scope;
    if (scope_freelist_n > 0) {
        scope = scope_freelist[--scope_freelist_n];
        _Py_NewReference((PyObject *)scope);
    } else {
        scope = PyObject_GC_New(Scope, &ScopeType);
        if (scope == NULL)
            return NULL;
    }
    Py_INCREF(fsm);
    scope->sc_fsm = fsm;
    scope->sc_listeners = NULL;
    scope->sc_timers = NULL;
    scope->sc_active = 1;
    scope->sc_nreg = 0;
    PyObject_GC_Track((PyObject *)scope);
    return scope;
}

/* guarded zero/N-arg callback: no-op once scope inactive */
typedef struct {
    PyObject_HEAD
    PyObject *gc_scope;   /* Scope* */
    PyObject *gc_cb;
} GuardedCb;

extern PyTypeObject GuardedCbType;

PyObject *
GuardedCb_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    GuardedCb *self = (GuardedCb *)self_;
    (void)kwds;
    if (!((Scope *)self->gc_scope)->sc_active)
        Py_RETURN_NONE;
    return PyObject_Call(self->gc_cb, args, NULL);
}

int
GuardedCb_traverse(PyObject *self_, visitproc visit, void *arg)
{
    GuardedCb *self = (GuardedCb *)self_;
    Py_VISIT(self->gc_scope);
    Py_VISIT(self->gc_cb);
    return 0;
}

int
GuardedCb_clear_(PyObject *self_)
{
    GuardedCb *self = (GuardedCb *)self_;
    Py_CLEAR(self->gc_scope);
    Py_CLEAR(self->gc_cb);
    return 0;
}

void
GuardedCb_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    GuardedCb_clear_(self_);
    PyObject_GC_Del(self_);
}

PyTypeObject GuardedCbType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._GuardedCb",
    sizeof(GuardedCb),
    0,
    GuardedCb_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    GuardedCb_call,
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    0,
    GuardedCb_traverse,
    GuardedCb_clear_,
};

PyObject *
make_guarded(PyObject *scope, PyObject *cb)
{
    GuardedCb *g = PyObject_GC_New(GuardedCb, &GuardedCbType);
    if (g == NULL)
        return NULL;
    Py_INCREF(scope);
    g->gc_scope = scope;
    Py_INCREF(cb);
    g->gc_cb = cb;
    PyObject_GC_Track((PyObject *)g);
    return (PyObject *)g;
}

int
scope_check_active(Scope *self, const char *what)
{
    if (!self->sc_active) {
        PyErr_Format(g_fsm_error, "%s used on exited state scope", what);
        return -1;
    }
    return 0;
}

/* the registration core of S.on(), callable from C (SlotKit) */
int
scope_on_c(Scope *self, PyObject *emitter, PyObject *event, PyObject *cb)
{
    PyObject *r;
    if (Py_TYPE(emitter) == &EmitterType) {
        r = emitter_add((Emitter *)emitter, event, cb);
    } else {
        r = PyObject_CallMethodObjArgs(emitter, s_on, event, cb, NULL);
    }
    if (r == NULL)
        return -1;
    Py_DECREF(r);
    if (self->sc_nreg < SCOPE_INLINE_REGS) {
        PyObject **slot = self->sc_reg + 3 * self->sc_nreg;
        Py_INCREF(emitter);
        slot[0] = emitter;
        Py_INCREF(event);
        slot[1] = event;
        Py_INCREF(cb);
        slot[2] = cb;
        self->sc_nreg++;
        return 0;
    }
    if (self->sc_listeners == NULL) {
        self->sc_listeners = PyList_New(0);
        if (self->sc_listeners == NULL)
            return -1;
    }
    if (PyList_Append(self->sc_listeners, emitter) < 0 ||
        PyList_Append(self->sc_listeners, event) < 0 ||
        PyList_Append(self->sc_listeners, cb) < 0)
        return -1;
    return 0;
}

PyObject *
Scope_on(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    Scope *self = (Scope *)self_;
    if (nargs != 3) {
        PyErr_SetString(PyExc_TypeError, "S.on(emitter, event, cb)");
        return NULL;
    }
    if (scope_check_active(self, "S.on()") < 0)
        return NULL;
    if (scope_on_c(self, args[0], args[1], args[2]) < 0)
        return NULL;
    Py_RETURN_NONE;
}

int
scope_add_timer(Scope *self, PyObject *handle)
{
    if (self->sc_timers == NULL) {
        self->sc_timers = PyList_New(0);
        if (self->sc_timers == NULL)
            return -1;
    }
    return PyList_Append(self->sc_timers, handle);
}

PyObject *fsm_get_loop_of(FSMOb *fsm);

PyObject *
Scope_timeout(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    Scope *self = (Scope *)self_;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "S.timeout(ms, cb)");
        return NULL;
    }
    if (scope_check_active(self, "S.timeout()") < 0)
        return NULL;
    double ms = PyFloat_AsDouble(args[0]);
    if (ms == -1.0 && PyErr_Occurred())
        return NULL;
    PyObject *guarded = make_guarded(self_, args[1]);
    if (guarded == NULL)
        return NULL;
    PyObject *secs = PyFloat_FromDouble(ms / 1000.0);
    if (secs == NULL) {
        Py_DECREF(guarded);
        return NULL;
    }
    PyObject *loop = fsm_get_loop_of((FSMOb *)self->sc_fsm);
    PyObject *handle = PyObject_CallMethodObjArgs(loop, s_call_later, secs,
                                                  guarded, NULL);
    Py_DECREF(secs);
    Py_DECREF(guarded);
    if (handle == NULL)
        return NULL;
    int rc = scope_add_timer(self, handle);
    Py_DECREF(handle);
    if (rc < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
Scope_immediate(PyObject *self_, PyObject *cb)
{
    Scope *self = (Scope *)self_;
    if (scope_check_active(self, "S.immediate()") < 0)
        return NULL;
    PyObject *guarded = make_guarded(self_, cb);
    if (guarded == NULL)
        return NULL;
    PyObject *loop = fsm_get_loop_of((FSMOb *)self->sc_fsm);
    PyObject *handle = PyObject_CallMethodObjArgs(loop, s_call_soon,
                                                  guarded, NULL);
    Py_DECREF(guarded);
    if (handle == NULL)
        return NULL;
    int rc = scope_add_timer(self, handle);
    Py_DECREF(handle);
    if (rc < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
Scope_callback(PyObject *self_, PyObject *cb)
{
    Scope *self = (Scope *)self_;
    if (scope_check_active(self, "S.callback()") < 0)
        return NULL;
    return make_guarded(self_, cb);
}

PyObject *Scope_interval(PyObject *self_, PyObject *const *args,
                         Py_ssize_t nargs);

PyObject *
Scope_valid_transitions(PyObject *self_, PyObject *states);

PyObject *
Scope_goto_state(PyObject *self_, PyObject *state)
{
    Scope *self = (Scope *)self_;
    if (!self->sc_active)
        Py_RETURN_NONE;   /* stale handler during a cascade: obsolete */
    if (fsm_goto_state((FSMOb *)self->sc_fsm, state) < 0)
        return NULL;
    Py_RETURN_NONE;
}

/* the claim handle's own remove_listener (ClaimHandleBase section) */
PyObject *g_ch_remove_desc;
PyObject *CH_remove_listener(PyObject *self_, PyObject *const *args,
                             Py_ssize_t nargs);

/* undo one S.on() registration */
int
scope_unregister(PyObject *em, PyObject *evt, PyObject *cb)
{
    PyObject *r;
    /* fast path only when the type's MRO resolves remove_listener to
     * our own C method (no override) */
    int fast = 0;
    if (PyType_IsSubtype(Py_TYPE(em), &EmitterType)) {
        PyObject *desc = _PyType_Lookup(Py_TYPE(em), s_remove_listener);
        fast = (desc == g_remove_desc) ? 1
            : (desc != NULL && desc == g_ch_remove_desc) ? 2 : 0;
    }
    if (fast) {
        PyObject *cargs[2] = {evt, cb};
        r = fast == 1 ? Emitter_remove_listener(em, cargs, 2)
                      : CH_remove_listener(em, cargs, 2);
    } else {
        r = PyObject_CallMethodObjArgs(em, s_remove_listener, evt, cb,
                                       NULL);
    }
    if (r == NULL)
        return -1;
    Py_DECREF(r);
    return 0;
}

PyObject *
Scope_dispose(PyObject *self_, PyObject *noargs)
{
    Scope *self = (Scope *)self_;
    (void)noargs;
    self->sc_active = 0;
    /* take the registrations out first: removing a listener can run
     * arbitrary code, which may come back here */
    PyObject *regs[3 * SCOPE_INLINE_REGS];
    int nreg = self->sc_nreg;
    self->sc_nreg = 0;
    for (int i = 0; i < 3 * nreg; i++)
        regs[i] = self->sc_reg[i];
    PyObject *ls = self->sc_listeners;
    self->sc_listeners = NULL;
    int failed = 0;
    for (int i = 0; i < nreg; i++) {
        if (!failed &&
            scope_unregister(regs[3 * i], regs[3 * i + 1],
                             regs[3 * i + 2]) < 0)
            failed = 1;
        Py_DECREF(regs[3 * i]);
        Py_DECREF(regs[3 * i + 1]);
        Py_DECREF(regs[3 * i + 2]);
    }
    if (failed) {
        Py_XDECREF(ls);
        return NULL;
    }
    if (ls != NULL) {
        Py_ssize_t n = PyList_GET_SIZE(ls);
        for (Py_ssize_t i = 0; i + 2 < n; i += 3) {
            if (scope_unregister(PyList_GET_ITEM(ls, i),
                                 PyList_GET_ITEM(ls, i + 1),
                                 PyList_GET_ITEM(ls, i + 2)) < 0) {
                Py_DECREF(ls);
                return NULL;
            }
        }
        Py_DECREF(ls);
    }
    PyObject *ts = self->sc_timers;
    self->sc_timers = NULL;
    if (ts != NULL) {
        Py_ssize_t n = PyList_GET_SIZE(ts);
        for (Py_ssize_t i = 0; i < n; i++) {
            PyObject *r = PyObject_CallMethodObjArgs(
                PyList_GET_ITEM(ts, i), s_cancel, NULL);
            if (r == NULL) {
                Py_DECREF(ts);
                return NULL;
            }
            Py_DECREF(r);
        }
        Py_DECREF(ts);
    }
    Py_RETURN_NONE;
}

PyObject *
Scope_get_active(PyObject *self_, void *closure)
{
    (void)closure;
    return PyBool_FromLong(((Scope *)self_)->sc_active);
}

int
Scope_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Scope *self = (Scope *)self_;
    Py_VISIT(self->sc_fsm);
    Py_VISIT(self->sc_listeners);
    Py_VISIT(self->sc_timers);
    for (int i = 0; i < 3 * self->sc_nreg; i++)
        Py_VISIT(self->sc_reg[i]);
    return 0;
}

int
Scope_clear_(PyObject *self_)
{
    Scope *self = (Scope *)self_;
    Py_CLEAR(self->sc_fsm);
    Py_CLEAR(self->sc_listeners);
    Py_CLEAR(self->sc_timers);
    int nreg = self->sc_nreg;
    self->sc_nreg = 0;
    for (int i = 0; i < 3 * nreg; i++)
        Py_CLEAR(self->sc_reg[i]);
    return 0;
}

void
Scope_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    Scope_clear_(self_);
    if (scope_freelist_n < SCOPE_FREELIST_MAX)
        scope_freelist[scope_freelist_n++] = (Scope *)self_;
    else
        PyObject_GC_Del(self_);
}

PyMethodDef Scope_methods[] = {
    {"on", (PyCFunction)(void (*)(void))Scope_on, METH_FASTCALL, NULL},
    {"timeout", (PyCFunction)(void (*)(void))Scope_timeout, METH_FASTCALL,
     NULL},
    {"interval", (PyCFunction)(void (*)(void))Scope_interval,
     METH_FASTCALL, NULL},
    {"immediate", Scope_immediate, METH_O, NULL},
    {"callback", Scope_callback, METH_O, NULL},
    {"valid_transitions", Scope_valid_transitions, METH_O, NULL},
    {"goto_state", Scope_goto_state, METH_O, NULL},
    {"_dispose", Scope_dispose, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

PyGetSetDef Scope_getset[] = {
    {(char *)"active", Scope_get_active, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject ScopeType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.StateScope",
    sizeof(Scope),
    0,
    Scope_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    "FSM state scope (native)",
    Scope_traverse,
    Scope_clear_,
    0, 0, 0, 0,
    Scope_methods,
    0,
    Scope_getset,
};

/* ------------------------------------------------------------------ */
/* FSM                                                                 */
/* ------------------------------------------------------------------ */

struct FSMOb {
    Emitter base;
    PyObject *f_loop;
    PyObject *f_state;          /* str or NULL */
    PyObject *f_scope;          /* Scope* or NULL */
    PyObject *f_valid;          /* sequence or NULL */
    PyObject *f_pending;        /* str or NULL */
    /* queued stateChanged emissions, oldest at f_eq_head.  They live in
     * f_eq_inl until more than FSM_EQ_INLINE are pending at once, then
     * in a malloc'ed array; popping moves the head, and the array is
     * compacted once per flush */
    PyObject **f_eq;            /* f_eq_inl or heap */
    Py_ssize_t f_eq_head, f_eq_len, f_eq_cap;
    PyObject *f_eq_inl[4];
    /* the last FSM_HISTORY states as a ring; f_hist_n counts every
     * transition, the newest is at (f_hist_n - 1) % FSM_HISTORY */
    PyObject *f_hist[8];
    unsigned long f_hist_n;
    PyObject *f_flush_bound;    /* cached bound _flush_state_changed */
    PyObject *f_fastkit;        /* SlotKit* or NULL: native entries for
                                 * the busy/idle hot cycle */
    PyObject *f_watchkit;       /* SlotKit* or NULL, on a socket manager:
                                 * the kit whose slot reacts to this
                                 * FSM's stateChanged while busy or idle */
    PyObject *f_ctx;            /* PoolCtx* or NULL, on a pool: what the
                                 * claim cycle reads of it (pool_ctx) */
    int f_entering;
    int f_emit_scheduled;
    int f_own_reg;              /* a claim handle in `claimed` that holds its
                                 * connection's error registration itself
                                 * (ch_drop_conn_err) */
};

/* forward decl (SlotKit lives after the CH/Queue sections);
 * returns 1 = state entered natively, 0 = use the python entry,
 * -1 = error */
int slotkit_maybe_entry(PyObject *kit_, FSMOb *fsm, PyObject *target);
/* the watching kit's reaction to a stateChanged of its socket manager,
 * after the listeners in the list */
int slotkit_smgr_hook(PyObject *kit_, PyObject *st, unsigned long serial);
/* the kit's slot's transition count: taken before an emission, it tells
 * the hook afterwards whether the slot was in its state all along (a
 * listener registered during an emission is not called by it either) */
unsigned long slotkit_slot_serial(PyObject *kit_);
/* stateChanged of a claim handle: ticket hook, listeners, slot hook */
int ch_emit_state_changed(FSMOb *self, PyObject *st);

/* The scope of the current state, made on first use: most states of the
 * claim cycle register nothing.  Borrowed; NULL on error. */
static inline Scope *
fsm_need_scope(FSMOb *self)
{
    if (self->f_scope == NULL)
        self->f_scope = (PyObject *)scope_new((PyObject *)self);
    return (Scope *)self->f_scope;
}

/* claim-handle terminal cleanup (defined near the CH section) */
extern PyObject *t_empty;
extern PyTypeObject CHType;
extern PyTypeObject CTType;
void ch_terminal_cleanup(FSMOb *self);
/* leaving `claimed`: remove the error listener the handle registered on
 * its connection without a scope (f_own_reg) */
int ch_drop_conn_err(FSMOb *self);

/* the claim handle's C state entry for `target`, if the type of `self`
 * still resolves that entry to it (no Python override); else NULL */
typedef PyObject *(*ch_entry_fn)(PyObject *, PyObject *);
ch_entry_fn ch_direct_entry(FSMOb *self, PyObject *target);

extern PyTypeObject FSMType;
extern PyTypeObject SlotBaseType;

/* The objects of the claim cycle are instances of three Python classes
 * (ClaimHandle, ConnectionSlotFSM, ConnectionPool), never of the native
 * bases themselves, so PyObject_TypeCheck's exact-type shortcut misses
 * and every test walks the MRO.  The classes are registered at import
 * (owned references); a type that is none of them gets the walk. */
PyTypeObject *g_handle_cls;    /* connection_fsm.ClaimHandle */
PyTypeObject *g_slot_cls;      /* connection_fsm.ConnectionSlotFSM */
PyTypeObject *g_pool_cls;      /* pool.ConnectionPool */

static inline int
is_handle(PyObject *x)
{
#if CUEBALL_EXACT_TYPES
    if (Py_TYPE(x) == g_handle_cls)
        return 1;
#endif
    return PyObject_TypeCheck(x, &CHType);
}

static inline int
is_slot(PyObject *x)
{
#if CUEBALL_EXACT_TYPES
    if (Py_TYPE(x) == g_slot_cls)
        return 1;
#endif
    return PyObject_TypeCheck(x, &SlotBaseType);
}

static inline int
is_fsm(PyObject *x)
{
#if CUEBALL_EXACT_TYPES
    PyTypeObject *tp = Py_TYPE(x);
    if (tp == g_pool_cls || tp == g_slot_cls || tp == g_handle_cls)
        return 1;
#endif
    return PyObject_TypeCheck(x, &FSMType);
}

PyObject *
fsm_get_loop_of(FSMOb *fsm)
{
    return fsm->f_loop;
}

#define FSM_EQ_INLINE 4
#define FSM_HISTORY 8

static void
fsm_eq_compact(FSMOb *f)
{
    if (f->f_eq_head == 0)
        return;
    Py_ssize_t n = f->f_eq_len - f->f_eq_head;
    memmove(f->f_eq, f->f_eq + f->f_eq_head, n * sizeof(PyObject *));
    f->f_eq_head = 0;
    f->f_eq_len = n;
}

static int
fsm_eq_push(FSMOb *f, PyObject *st)
{
    if (f->f_eq == NULL) {
        f->f_eq = f->f_eq_inl;
        f->f_eq_cap = FSM_EQ_INLINE;
        f->f_eq_head = f->f_eq_len = 0;
    }
    if (f->f_eq_len == f->f_eq_cap) {
        if (f->f_eq_head > 0) {
            fsm_eq_compact(f);
        } else {
            Py_ssize_t ncap = f->f_eq_cap * 2;
            PyObject **items;
            if (f->f_eq == f->f_eq_inl) {
                items = (PyObject **)PyMem_Malloc(
                    ncap * sizeof(PyObject *));
                if (items != NULL)
                    memcpy(items, f->f_eq_inl, sizeof(f->f_eq_inl));
            } else {
                items = (PyObject **)PyMem_Realloc(
                    f->f_eq, ncap * sizeof(PyObject *));
            }
            if (items == NULL) {
                PyErr_NoMemory();
                return -1;
            }
            f->f_eq = items;
            f->f_eq_cap = ncap;
        }
    }
    Py_INCREF(st);
    f->f_eq[f->f_eq_len++] = st;
    return 0;
}

static void
fsm_eq_clear(FSMOb *f)
{
    PyObject **items = f->f_eq;
    Py_ssize_t head = f->f_eq_head, len = f->f_eq_len;
    f->f_eq = NULL;
    f->f_eq_head = f->f_eq_len = f->f_eq_cap = 0;
    if (items == NULL)
        return;
    for (Py_ssize_t i = head; i < len; i++)
        Py_DECREF(items[i]);
    if (items != f->f_eq_inl)
        PyMem_Free(items);
}

int fsm_schedule_flush(FSMOb *self);

/* Per-FSM drain cap: one FSM whose listeners keep triggering its own
 * transitions would otherwise drain forever inside a single loop
 * callback (the batch cap only bounds distinct flush entries).  The
 * remainder is rescheduled in order. */
#define FSM_FLUSH_CAP 64

int
fsm_flush_core(FSMOb *self)
{
    self->f_emit_scheduled = 0;
    int n = 0;
    int handle = is_handle((PyObject *)self);
    while (self->f_eq_head < self->f_eq_len && n++ < FSM_FLUSH_CAP) {
        /* pop by index; listeners may queue more (or flush again)
         * while they run, so the queue is read afresh every turn */
        PyObject *st = self->f_eq[self->f_eq_head++];
        if (self->f_eq_head == self->f_eq_len)
            self->f_eq_head = self->f_eq_len = 0;
        int r;
        if (handle) {
            r = ch_emit_state_changed(self, st);
        } else {
            PyObject *eargs[2] = {s_stateChanged, st};
            unsigned long serial = self->f_watchkit == NULL ? 0
                : slotkit_slot_serial(self->f_watchkit);
            r = emitter_emit_core(&self->base, eargs[0], eargs + 1, 1);
            if (r >= 0 && serial != 0 && self->f_watchkit != NULL &&
                slotkit_smgr_hook(self->f_watchkit, st, serial) < 0)
                r = -1;
        }
        Py_DECREF(st);
        if (r < 0) {
            fsm_eq_compact(self);
            return -1;
        }
    }
    fsm_eq_compact(self);
    if (self->f_eq_len > 0 && !self->f_emit_scheduled)
        return fsm_schedule_flush(self);
    return 0;
}

PyObject *
FSM_flush_state_changed(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    if (fsm_flush_core((FSMOb *)self_) < 0)
        return NULL;
    Py_RETURN_NONE;
}

/* Batched flush: all FSMs that queue a stateChanged in the same loop
 * turn share one call_soon.  Relative order is preserved (FSMs drain in
 * first-queue order; each FSM drains its whole queue, exactly as the
 * per-FSM call_soon did).  While the batch is draining it stays
 * registered, so FSMs that queue *during* the drain (the serial
 * claim-chain case: a flush completes one claim cycle, whose callback
 * immediately starts the next claim) are appended to the same batch
 * and drained in the same loop callback.  That collapses long
 * callback-chained sequences into one event-loop turn instead of one
 * turn (epoll_wait + ready-queue bookkeeping) per link.  The drain is
 * capped per callback so a self-sustaining chain cannot starve IO; the
 * remainder is rescheduled with a fresh call_soon. */
#define FLUSH_DRAIN_CAP 48

typedef struct {
    PyObject_HEAD
    PyObject *fb_loop;
    PyObject *fb_list;   /* list of FSMOb */
    Py_ssize_t fb_pos;   /* next index to drain */
    vectorcallfunc fb_vectorcall;
} FlushBatch;

extern PyTypeObject FlushBatchType;

static void
flushbatch_detach(FlushBatch *self)
{
    PyObject *cur = PyDict_GetItemWithError(g_flush_batches, self->fb_loop);
    if (cur == (PyObject *)self)
        (void)PyDict_DelItem(g_flush_batches, self->fb_loop);
    else if (cur == NULL)
        PyErr_Clear();
}

static PyObject *
flushbatch_run(PyObject *self_)
{
    FlushBatch *self = (FlushBatch *)self_;
    int rounds = 0;
    while (self->fb_pos < PyList_GET_SIZE(self->fb_list) &&
           rounds < FLUSH_DRAIN_CAP) {
        FSMOb *fsm = (FSMOb *)PyList_GET_ITEM(self->fb_list,
                                              self->fb_pos);
        self->fb_pos++;
        rounds++;
        if (fsm_flush_core(fsm) < 0) {
            /* un-wedge the FSMs we did not get to: their next
             * emission must be able to schedule a flush again */
            for (Py_ssize_t i = self->fb_pos;
                 i < PyList_GET_SIZE(self->fb_list); i++) {
                FSMOb *f = (FSMOb *)PyList_GET_ITEM(self->fb_list, i);
                f->f_emit_scheduled = 0;
            }
            flushbatch_detach(self);
            return NULL;
        }
    }
    if (self->fb_pos < PyList_GET_SIZE(self->fb_list)) {
        /* cap hit: yield to the loop, keep the batch registered so
         * new queuers keep appending, and finish on the next turn.
         * Compact the drained prefix first — under sustained load the
         * batch never empties and would otherwise grow without bound. */
        if (PyList_SetSlice(self->fb_list, 0, self->fb_pos, NULL) < 0) {
            flushbatch_detach(self);
            return NULL;
        }
        self->fb_pos = 0;
        PyObject *h = PyObject_CallMethodObjArgs(
            self->fb_loop, s_call_soon, self_, NULL);
        if (h == NULL) {
            flushbatch_detach(self);
            return NULL;
        }
        Py_DECREF(h);
        Py_RETURN_NONE;
    }
    flushbatch_detach(self);
    Py_RETURN_NONE;
}

PyObject *
FlushBatch_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    (void)args; (void)kwds;
    return flushbatch_run(self_);
}

/* the event loop calls the batch with no arguments: no tuple is built */
static PyObject *
FlushBatch_vectorcall(PyObject *self_, PyObject *const *args, size_t nargsf,
                      PyObject *kwnames)
{
    (void)args; (void)nargsf; (void)kwnames;
    return flushbatch_run(self_);
}

int
FlushBatch_traverse(PyObject *self_, visitproc visit, void *arg)
{
    FlushBatch *self = (FlushBatch *)self_;
    Py_VISIT(self->fb_loop);
    Py_VISIT(self->fb_list);
    return 0;
}

int
FlushBatch_clear_(PyObject *self_)
{
    FlushBatch *self = (FlushBatch *)self_;
    Py_CLEAR(self->fb_loop);
    Py_CLEAR(self->fb_list);
    return 0;
}

void
FlushBatch_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    FlushBatch_clear_(self_);
    PyObject_GC_Del(self_);
}

PyTypeObject FlushBatchType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._FlushBatch",
    sizeof(FlushBatch),
    0,
    FlushBatch_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    FlushBatch_call,              /* vectorcall: see slotkit_types_init */
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    0,
    FlushBatch_traverse,
    FlushBatch_clear_,
};

int
fsm_queue_state_changed(FSMOb *self, PyObject *state)
{
    if (fsm_eq_push(self, state) < 0)
        return -1;
    return fsm_schedule_flush(self);
}

int
fsm_schedule_flush(FSMOb *self)
{
    if (self->f_emit_scheduled)
        return 0;
    self->f_emit_scheduled = 1;
    PyObject *batch = PyDict_GetItemWithError(g_flush_batches, self->f_loop);
    if (batch == NULL) {
        if (PyErr_Occurred())
            return -1;
        FlushBatch *fb = PyObject_GC_New(FlushBatch, &FlushBatchType);
        if (fb == NULL)
            return -1;
        Py_INCREF(self->f_loop);
        fb->fb_loop = self->f_loop;
        fb->fb_pos = 0;
        fb->fb_vectorcall = FlushBatch_vectorcall;
        fb->fb_list = PyList_New(0);
        PyObject_GC_Track((PyObject *)fb);
        if (fb->fb_list == NULL) {
            Py_DECREF(fb);
            return -1;
        }
        if (PyDict_SetItem(g_flush_batches, self->f_loop,
                           (PyObject *)fb) < 0) {
            Py_DECREF(fb);
            return -1;
        }
        PyObject *h = PyObject_CallMethodObjArgs(
            self->f_loop, s_call_soon, (PyObject *)fb, NULL);
        if (h == NULL) {
            Py_DECREF(fb);
            return -1;
        }
        Py_DECREF(h);
        batch = (PyObject *)fb;
        Py_DECREF(fb);  /* dict holds it */
    }
    if (PyList_Append(((FlushBatch *)batch)->fb_list,
                      (PyObject *)self) < 0)
        return -1;
    return 0;
}

/* resolve "state_x_y" attr name for a state string, cached globally */
PyObject *
entry_attr_name(PyObject *state)
{
    PyObject *name = PyDict_GetItemWithError(g_entry_name_cache, state);
    if (name != NULL) {
        Py_INCREF(name);
        return name;
    }
    if (PyErr_Occurred())
        return NULL;
    PyObject *replaced = PyObject_CallMethod(state, "replace", "OO",
                                             s_dot, s_underscore);
    if (replaced == NULL)
        return NULL;
    name = PyUnicode_Concat(s_state_prefix, replaced);
    Py_DECREF(replaced);
    if (name == NULL)
        return NULL;
    PyUnicode_InternInPlace(&name);
    if (PyDict_SetItem(g_entry_name_cache, state, name) < 0) {
        Py_DECREF(name);
        return NULL;
    }
    return name;
}

int
check_valid(FSMOb *self, PyObject *from, PyObject *state)
{
    if (self->f_valid == NULL)
        return 0;
#if CUEBALL_VALID_IDENTITY
    /* the native cycle's f_valid is one of this module's constant tuples
     * and `state` one of its interned names: found by identity, no rich
     * compare.  Anything else (a list, an equal string that is another
     * object, a miss) is answered by the sequence protocol as before. */
    if (PyTuple_CheckExact(self->f_valid)) {
        PyObject *v = self->f_valid;
        for (Py_ssize_t i = 0, n = PyTuple_GET_SIZE(v); i < n; i++)
            if (PyTuple_GET_ITEM(v, i) == state)
                return 0;
    }
#endif
    int c = PySequence_Contains(self->f_valid, state);
    if (c < 0)
        return -1;
    if (!c) {
        PyErr_Format(g_fsm_error,
                     "%s: invalid transition %R -> %R (valid: %R)",
                     Py_TYPE(self)->tp_name,
                     from ? from : Py_None, state, self->f_valid);
        return -1;
    }
    return 0;
}

int
fsm_enter_loop(FSMOb *self, PyObject *state)
{
    PyObject *next_state = state;
    Py_INCREF(next_state);
    while (next_state != NULL) {
        PyObject *target = next_state;
        next_state = NULL;
        if (self->f_scope != NULL) {
            PyObject *old = self->f_scope;
            self->f_scope = NULL;
            PyObject *r = Scope_dispose(old, NULL);
            Py_DECREF(old);
            if (r == NULL) {
                Py_DECREF(target);
                return -1;
            }
            Py_DECREF(r);
        }
        if (self->f_own_reg && ch_drop_conn_err(self) < 0) {
            Py_DECREF(target);
            return -1;
        }
        Py_CLEAR(self->f_valid);
        Py_INCREF(target);
        Py_XSETREF(self->f_state, target);
        Py_INCREF(target);
        Py_XSETREF(self->f_hist[self->f_hist_n % FSM_HISTORY], target);
        self->f_hist_n++;
#if !CUEBALL_LAZY_SCOPES
        if (fsm_need_scope(self) == NULL) {
            Py_DECREF(target);
            return -1;
        }
#endif

        if (g_tracer != NULL && g_tracer != Py_None) {
            PyObject *targs[2] = {(PyObject *)self, target};
            PyObject *tr = PyObject_Vectorcall(g_tracer, targs, 2, NULL);
            if (tr == NULL) {
                Py_DECREF(target);
                return -1;
            }
            Py_DECREF(tr);
        }

        /* The native entries take the state's scope from fsm_need_scope()
         * if they register anything; a Python entry is handed one. */
        int handled = 0;
        if (self->f_fastkit != NULL) {
            self->f_entering = 1;
            handled = slotkit_maybe_entry(self->f_fastkit, self, target);
            self->f_entering = 0;
            if (handled < 0) {
                Py_DECREF(target);
                return -1;
            }
        }
        PyObject *r;
        ch_entry_fn direct = handled ? NULL : ch_direct_entry(self, target);
        if (handled) {
            r = Py_None;
            Py_INCREF(r);
        } else if (direct != NULL) {
            /* the type's entry for this state is this module's own C
             * function: call it without building a bound method */
            self->f_entering = 1;
            r = direct((PyObject *)self, NULL);
            self->f_entering = 0;
        } else {
            PyObject *attr = entry_attr_name(target);
            if (attr == NULL) {
                Py_DECREF(target);
                return -1;
            }
            PyObject *entry = PyObject_GetAttr((PyObject *)self, attr);
            Py_DECREF(attr);
            if (entry == NULL) {
                PyErr_Clear();
                PyErr_Format(g_fsm_error,
                             "%s has no state-entry function for %R",
                             Py_TYPE(self)->tp_name, target);
                Py_DECREF(target);
                return -1;
            }
            PyObject *scope = (PyObject *)fsm_need_scope(self);
            if (scope == NULL) {
                Py_DECREF(entry);
                Py_DECREF(target);
                return -1;
            }
            Py_INCREF(scope);
            self->f_entering = 1;
            r = PyObject_CallOneArg(entry, scope);
            Py_DECREF(entry);
            Py_DECREF(scope);
            self->f_entering = 0;
        }
        PyObject *pend = self->f_pending;
        self->f_pending = NULL;
        if (r == NULL) {
            Py_XDECREF(pend);
            Py_DECREF(target);
            return -1;
        }
        Py_DECREF(r);
        if (fsm_queue_state_changed(self, target) < 0) {
            Py_XDECREF(pend);
            Py_DECREF(target);
            return -1;
        }
        if (pend != NULL) {
            if (check_valid(self, target, pend) < 0) {
                Py_DECREF(pend);
                Py_DECREF(target);
                return -1;
            }
            next_state = pend;
        }
        Py_DECREF(target);
    }
    /* Settled in a claim-handle terminal state (they mark themselves
     * with the shared empty valid-transitions tuple): break the
     * per-claim reference cycles — fsm<->scope and handle<->ticket —
     * so the whole claim's object graph is freed by reference
     * counting.  Without this every claim leaves cyclic garbage and
     * CPython's cyclic GC pauses dominate claim p99 (measured 4x). */
    if (self->f_valid == t_empty &&
        is_handle((PyObject *)self))
        ch_terminal_cleanup(self);
    return 0;
}

int
fsm_goto_state(FSMOb *self, PyObject *state)
{
    if (check_valid(self, self->f_state, state) < 0)
        return -1;
    if (self->f_entering) {
        if (self->f_pending != NULL) {
            int eq = PyObject_RichCompareBool(self->f_pending, state, Py_EQ);
            if (eq < 0)
                return -1;
            if (!eq) {
                PyErr_Format(g_fsm_error,
                             "%s: conflicting deferred transitions %R and "
                             "%R from %R", Py_TYPE(self)->tp_name,
                             self->f_pending, state,
                             self->f_state ? self->f_state : Py_None);
                return -1;
            }
            return 0;
        }
        Py_INCREF(state);
        self->f_pending = state;
        return 0;
    }
    return fsm_enter_loop(self, state);
}

int
FSM_init(PyObject *self_, PyObject *args, PyObject *kwds)
{
    FSMOb *self = (FSMOb *)self_;
    PyObject *initial = NULL, *loop = Py_None;
    static const char *kwlist[] = {"initial_state", "loop", NULL};
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "U|O",
                                     const_cast<char **>(kwlist),
                                     &initial, &loop))
        return -1;
    if (Emitter_init(self_, NULL, NULL) < 0)
        return -1;
    PyObject *resolved = resolve_loop(loop);
    if (resolved == NULL)
        return -1;
    Py_XSETREF(self->f_loop, resolved);
    Py_CLEAR(self->f_state);
    Py_CLEAR(self->f_valid);
    Py_CLEAR(self->f_pending);
    self->f_entering = 0;
    return fsm_goto_state(self, initial);
}

PyObject *
FSM_get_state(PyObject *self_, PyObject *noargs)
{
    FSMOb *self = (FSMOb *)self_;
    (void)noargs;
    if (self->f_state == NULL) {
        PyErr_SetString(g_fsm_error, "FSM has no state yet");
        return NULL;
    }
    Py_INCREF(self->f_state);
    return self->f_state;
}

PyObject *
FSM_is_in_state(PyObject *self_, PyObject *state)
{
    FSMOb *self = (FSMOb *)self_;
    if (self->f_state == NULL)
        Py_RETURN_FALSE;
    int eq = PyUnicode_Compare(self->f_state, state);
    if (eq == -1 && PyErr_Occurred())
        return NULL;
    if (eq == 0)
        Py_RETURN_TRUE;
    /* prefix semantics: cur startswith state + "." */
    Py_ssize_t sl = PyUnicode_GET_LENGTH(state);
    Py_ssize_t cl = PyUnicode_GET_LENGTH(self->f_state);
    if (cl > sl) {
        int m = PyUnicode_Tailmatch(self->f_state, state, 0, sl, -1);
        if (m < 0)
            return NULL;
        if (m && PyUnicode_ReadChar(self->f_state, sl) == '.')
            Py_RETURN_TRUE;
    }
    Py_RETURN_FALSE;
}

PyObject *
FSM_get_state_history(PyObject *self_, PyObject *noargs)
{
    FSMOb *self = (FSMOb *)self_;
    (void)noargs;
    Py_ssize_t count = self->f_hist_n < FSM_HISTORY
        ? (Py_ssize_t)self->f_hist_n : FSM_HISTORY;
    PyObject *out = PyList_New(count);
    if (out == NULL)
        return NULL;
    unsigned long first = self->f_hist_n - (unsigned long)count;
    for (Py_ssize_t i = 0; i < count; i++) {
        PyObject *st = self->f_hist[(first + (unsigned long)i) %
                                    FSM_HISTORY];
        Py_INCREF(st);
        PyList_SET_ITEM(out, i, st);
    }
    return out;
}

PyObject *
FSM_goto_state_py(PyObject *self_, PyObject *state)
{
    if (!PyUnicode_Check(state)) {
        PyErr_SetString(PyExc_TypeError, "state must be a str");
        return NULL;
    }
    if (fsm_goto_state((FSMOb *)self_, state) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
FSM_get__fsm_state(PyObject *self_, void *closure)
{
    FSMOb *self = (FSMOb *)self_;
    (void)closure;
    if (self->f_state == NULL)
        Py_RETURN_NONE;
    Py_INCREF(self->f_state);
    return self->f_state;
}

PyObject *
FSM_get__fsm_valid(PyObject *self_, void *closure)
{
    FSMOb *self = (FSMOb *)self_;
    (void)closure;
    if (self->f_valid == NULL)
        Py_RETURN_NONE;
    Py_INCREF(self->f_valid);
    return self->f_valid;
}

int
FSM_set__fsm_valid(PyObject *self_, PyObject *value, void *closure)
{
    FSMOb *self = (FSMOb *)self_;
    (void)closure;
    if (value == NULL || value == Py_None) {
        Py_CLEAR(self->f_valid);
        return 0;
    }
    Py_INCREF(value);
    Py_XSETREF(self->f_valid, value);
    return 0;
}

PyObject *
Scope_valid_transitions(PyObject *self_, PyObject *states)
{
    Scope *self = (Scope *)self_;
    FSMOb *fsm = (FSMOb *)self->sc_fsm;
    Py_INCREF(states);
    Py_XSETREF(fsm->f_valid, states);
    Py_RETURN_NONE;
}

/* S.interval implemented natively with a tiny repeating driver */
typedef struct {
    PyObject_HEAD
    PyObject *iv_scope;
    PyObject *iv_cb;
    PyObject *iv_secs;
    PyObject *iv_handle;   /* current timer handle */
    int iv_stopped;
} IntervalOb;

extern PyTypeObject IntervalType;

PyObject *
Interval_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    IntervalOb *self = (IntervalOb *)self_;
    (void)args; (void)kwds;
    if (self->iv_stopped || !((Scope *)self->iv_scope)->sc_active)
        Py_RETURN_NONE;
    PyObject *r = PyObject_CallNoArgs(self->iv_cb);
    if (r == NULL)
        return NULL;
    Py_DECREF(r);
    if (!self->iv_stopped && ((Scope *)self->iv_scope)->sc_active) {
        FSMOb *fsm = (FSMOb *)((Scope *)self->iv_scope)->sc_fsm;
        PyObject *h = PyObject_CallMethodObjArgs(
            fsm->f_loop, s_call_later, self->iv_secs, self_, NULL);
        if (h == NULL)
            return NULL;
        Py_XSETREF(self->iv_handle, h);
    }
    Py_RETURN_NONE;
}

PyObject *
Interval_cancel(PyObject *self_, PyObject *noargs)
{
    IntervalOb *self = (IntervalOb *)self_;
    (void)noargs;
    self->iv_stopped = 1;
    if (self->iv_handle != NULL) {
        PyObject *r = PyObject_CallMethodObjArgs(self->iv_handle, s_cancel,
                                                 NULL);
        if (r == NULL)
            return NULL;
        Py_DECREF(r);
    }
    Py_RETURN_NONE;
}

int
Interval_traverse(PyObject *self_, visitproc visit, void *arg)
{
    IntervalOb *self = (IntervalOb *)self_;
    Py_VISIT(self->iv_scope);
    Py_VISIT(self->iv_cb);
    Py_VISIT(self->iv_handle);
    return 0;
}

int
Interval_clear_(PyObject *self_)
{
    IntervalOb *self = (IntervalOb *)self_;
    Py_CLEAR(self->iv_scope);
    Py_CLEAR(self->iv_cb);
    Py_CLEAR(self->iv_secs);
    Py_CLEAR(self->iv_handle);
    return 0;
}

void
Interval_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    Interval_clear_(self_);
    PyObject_GC_Del(self_);
}

PyMethodDef Interval_methods[] = {
    {"cancel", Interval_cancel, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

PyTypeObject IntervalType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._Interval",
    sizeof(IntervalOb),
    0,
    Interval_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    Interval_call,
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    0,
    Interval_traverse,
    Interval_clear_,
    0, 0, 0, 0,
    Interval_methods,
};

PyObject *
Scope_interval(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    Scope *self = (Scope *)self_;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "S.interval(ms, cb)");
        return NULL;
    }
    if (scope_check_active(self, "S.interval()") < 0)
        return NULL;
    double ms = PyFloat_AsDouble(args[0]);
    if (ms == -1.0 && PyErr_Occurred())
        return NULL;
    IntervalOb *iv = PyObject_GC_New(IntervalOb, &IntervalType);
    if (iv == NULL)
        return NULL;
    Py_INCREF(self_);
    iv->iv_scope = self_;
    Py_INCREF(args[1]);
    iv->iv_cb = args[1];
    iv->iv_secs = PyFloat_FromDouble(ms / 1000.0);
    iv->iv_handle = NULL;
    iv->iv_stopped = 0;
    PyObject_GC_Track((PyObject *)iv);
    if (iv->iv_secs == NULL) {
        Py_DECREF(iv);
        return NULL;
    }
    FSMOb *fsm = (FSMOb *)self->sc_fsm;
    PyObject *h = PyObject_CallMethodObjArgs(fsm->f_loop, s_call_later,
                                             iv->iv_secs, (PyObject *)iv,
                                             NULL);
    if (h == NULL) {
        Py_DECREF(iv);
        return NULL;
    }
    iv->iv_handle = h;
    int rc = scope_add_timer(self, (PyObject *)iv);
    Py_DECREF(iv);
    if (rc < 0)
        return NULL;
    Py_RETURN_NONE;
}

int
FSM_traverse(PyObject *self_, visitproc visit, void *arg)
{
    FSMOb *self = (FSMOb *)self_;
    Py_VISIT(self->f_loop);
    Py_VISIT(self->f_state);
    Py_VISIT(self->f_scope);
    Py_VISIT(self->f_valid);
    Py_VISIT(self->f_pending);
    for (Py_ssize_t i = self->f_eq_head; i < self->f_eq_len; i++)
        Py_VISIT(self->f_eq[i]);
    for (int i = 0; i < FSM_HISTORY; i++)
        Py_VISIT(self->f_hist[i]);
    Py_VISIT(self->f_flush_bound);
    Py_VISIT(self->f_fastkit);
    Py_VISIT(self->f_watchkit);
    Py_VISIT(self->f_ctx);
    return Emitter_traverse(self_, visit, arg);
}

int
FSM_clear_(PyObject *self_)
{
    FSMOb *self = (FSMOb *)self_;
    Py_CLEAR(self->f_loop);
    Py_CLEAR(self->f_state);
    Py_CLEAR(self->f_scope);
    Py_CLEAR(self->f_valid);
    Py_CLEAR(self->f_pending);
    fsm_eq_clear(self);
    for (int i = 0; i < FSM_HISTORY; i++)
        Py_CLEAR(self->f_hist[i]);
    self->f_hist_n = 0;
    Py_CLEAR(self->f_flush_bound);
    Py_CLEAR(self->f_fastkit);
    Py_CLEAR(self->f_watchkit);
    Py_CLEAR(self->f_ctx);
    return Emitter_clear_(self_);
}

void
FSM_dealloc(PyObject *self_)
{
    FSMOb *self = (FSMOb *)self_;
    PyTypeObject *tp = Py_TYPE(self_);
    PyObject_GC_UnTrack(self_);
    if (self->base.ev_weakrefs != NULL)
        PyObject_ClearWeakRefs(self_);
    FSM_clear_(self_);
    tp->tp_free(self_);
}

static PyObject *
FSM_set_fast_kit(PyObject *self_, PyObject *kit)
{
    FSMOb *self = (FSMOb *)self_;
    if (kit == Py_None) {
        Py_CLEAR(self->f_fastkit);
    } else {
        Py_INCREF(kit);
        Py_XSETREF(self->f_fastkit, kit);
    }
    Py_RETURN_NONE;
}

PyMethodDef FSM_methods[] = {
    {"get_state", FSM_get_state, METH_NOARGS, NULL},
    {"is_in_state", FSM_is_in_state, METH_O, NULL},
    {"get_state_history", FSM_get_state_history, METH_NOARGS, NULL},
    {"goto_state", FSM_goto_state_py, METH_O, NULL},
    {"_flush_state_changed", FSM_flush_state_changed, METH_NOARGS, NULL},
    {"_set_fast_kit", FSM_set_fast_kit, METH_O, NULL},
    {NULL, NULL, 0, NULL},
};

PyMemberDef FSM_members[] = {
    {(char *)"_loop", T_OBJECT, offsetof(FSMOb, f_loop), READONLY, NULL},
    {NULL, 0, 0, 0, NULL},
};

/* a pool's claim context, None until its first native claim or dispatch */
PyObject *
FSM_get__claim_ctx(PyObject *self_, void *closure)
{
    PyObject *cx = ((FSMOb *)self_)->f_ctx;
    (void)closure;
    if (cx == NULL)
        Py_RETURN_NONE;
    Py_INCREF(cx);
    return cx;
}

PyGetSetDef FSM_getset[] = {
    {(char *)"_fsm_state", FSM_get__fsm_state, NULL, NULL, NULL},
    {(char *)"_fsm_valid", FSM_get__fsm_valid, FSM_set__fsm_valid, NULL,
     NULL},
    {(char *)"_claim_ctx", FSM_get__claim_ctx, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject FSMType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.FSM",
    sizeof(FSMOb),
    0,
    FSM_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE | Py_TPFLAGS_HAVE_GC,
    "Moore machine (native)",
    FSM_traverse,
    FSM_clear_,
    0, 0, 0, 0,
    FSM_methods,
    FSM_members,
    FSM_getset,
    &EmitterType,                         /* tp_base */
    0, 0, 0,
    0,                                    /* tp_dictoffset (inherited) */
    FSM_init,
    0,
    PyType_GenericNew,
};

/* ------------------------------------------------------------------ */
/* SlotBase: native base of ConnectionSlotFSM.  It only holds the      */
/* fields that the claim cycle reads and writes from C several times   */
/* per claim, as struct members under their Python names, so neither   */
/* side goes through the instance dict for them.  An unset field reads */
/* as None.  The flags are objects: any truthy value works.            */

typedef struct {
    FSMOb base;
    PyObject *sl_handle;        /* csf_handle */
    PyObject *sl_prev_handle;   /* csf_prev_handle */
    PyObject *sl_wanted;        /* csf_wanted */
    PyObject *sl_monitor;       /* csf_monitor */
    PyObject *sl_idleq_node;    /* p_idleq_node */
    PyObject *sl_initq_node;    /* p_initq_node */
} SlotOb;

extern PyTypeObject SlotBaseType;

static inline int
slot_field_set(PyObject **field)
{
    return *field != NULL && *field != Py_None;
}

static inline int
slot_field_true(PyObject **field)
{
    PyObject *v = *field;
    if (v == Py_True)
        return 1;
    if (v == NULL || v == Py_False || v == Py_None)
        return 0;
    Py_INCREF(v);
    int t = PyObject_IsTrue(v);
    Py_DECREF(v);
    return t;
}

static inline void
slot_field_store(PyObject **field, PyObject *value)
{
    Py_XINCREF(value);
    Py_XSETREF(*field, value);
}

int
Slot_traverse(PyObject *self_, visitproc visit, void *arg)
{
    SlotOb *self = (SlotOb *)self_;
    Py_VISIT(self->sl_handle);
    Py_VISIT(self->sl_prev_handle);
    Py_VISIT(self->sl_wanted);
    Py_VISIT(self->sl_monitor);
    Py_VISIT(self->sl_idleq_node);
    Py_VISIT(self->sl_initq_node);
    return FSM_traverse(self_, visit, arg);
}

int
Slot_clear_(PyObject *self_)
{
    SlotOb *self = (SlotOb *)self_;
    Py_CLEAR(self->sl_handle);
    Py_CLEAR(self->sl_prev_handle);
    Py_CLEAR(self->sl_wanted);
    Py_CLEAR(self->sl_monitor);
    Py_CLEAR(self->sl_idleq_node);
    Py_CLEAR(self->sl_initq_node);
    return FSM_clear_(self_);
}

void
Slot_dealloc(PyObject *self_)
{
    SlotOb *self = (SlotOb *)self_;
    PyTypeObject *tp = Py_TYPE(self_);
    PyObject_GC_UnTrack(self_);
    if (self->base.base.ev_weakrefs != NULL)
        PyObject_ClearWeakRefs(self_);
    Slot_clear_(self_);
    tp->tp_free(self_);
}

PyMemberDef Slot_members[] = {
    {(char *)"csf_handle", T_OBJECT, offsetof(SlotOb, sl_handle), 0, NULL},
    {(char *)"csf_prev_handle", T_OBJECT, offsetof(SlotOb, sl_prev_handle),
     0, NULL},
    {(char *)"csf_wanted", T_OBJECT, offsetof(SlotOb, sl_wanted), 0, NULL},
    {(char *)"csf_monitor", T_OBJECT, offsetof(SlotOb, sl_monitor), 0,
     NULL},
    {(char *)"p_idleq_node", T_OBJECT, offsetof(SlotOb, sl_idleq_node), 0,
     NULL},
    {(char *)"p_initq_node", T_OBJECT, offsetof(SlotOb, sl_initq_node), 0,
     NULL},
    {NULL, 0, 0, 0, NULL},
};

PyTypeObject SlotBaseType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.SlotBase",
    sizeof(SlotOb),
    0,
    Slot_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE | Py_TPFLAGS_HAVE_GC,
    "connection slot FSM (native fields)",
    Slot_traverse,
    Slot_clear_,
    0, 0, 0, 0,
    0,
    Slot_members,
    0,
    &FSMType,
    0, 0, 0,
    0,
    0,                                    /* tp_init (inherited) */
    0,
    PyType_GenericNew,
};


/* ------------------------------------------------------------------ */
/* LatencyHistogram / PoolLatency: per-pool claim latency recording.   */
/* The arithmetic lives in lathist.h (no Python.h, so it is also       */
/* checked stand-alone); these are the Python faces.  The claim handle */
/* records into a PoolLatency straight from its state entries: one     */
/* clock read and one bucket increment, no allocation.                 */

typedef struct {
    PyObject_HEAD
    lathist::Hist h;
} LatHistOb;

extern PyTypeObject LatHistType;

static PyObject *
LatHist_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    (void)args; (void)kwds;
    LatHistOb *self = (LatHistOb *)type->tp_alloc(type, 0);
    if (self != NULL)
        self->h.reset();
    return (PyObject *)self;
}

static PyObject *
LatHist_record(PyObject *self_, PyObject *ms_)
{
    double ms = PyFloat_AsDouble(ms_);
    if (ms == -1.0 && PyErr_Occurred())
        return NULL;
    ((LatHistOb *)self_)->h.record_ms(ms);
    Py_RETURN_NONE;
}

static PyObject *
LatHist_counts(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    const lathist::Hist &h = ((LatHistOb *)self_)->h;
    PyObject *ls = PyList_New(lathist::NBUCKETS);
    if (ls == NULL)
        return NULL;
    for (int i = 0; i < lathist::NBUCKETS; i++) {
        PyObject *v = PyLong_FromUnsignedLongLong(h.counts[i]);
        if (v == NULL) {
            Py_DECREF(ls);
            return NULL;
        }
        PyList_SET_ITEM(ls, i, v);
    }
    return ls;
}

static PyObject *
lathist_percentile(const lathist::Hist &h, double q)
{
    if (h.count == 0)
        Py_RETURN_NONE;
    return PyFloat_FromDouble((double)h.percentile_us(q) / 1000.0);
}

static PyObject *
LatHist_percentile(PyObject *self_, PyObject *q_)
{
    double q = PyFloat_AsDouble(q_);
    if (q == -1.0 && PyErr_Occurred())
        return NULL;
    return lathist_percentile(((LatHistOb *)self_)->h, q);
}

/* cumulative(bounds_us) -> [samples with rounded us < bound, ...];
 * every bound must be a bucket boundary for the counts to be exact */
static PyObject *
LatHist_cumulative(PyObject *self_, PyObject *bounds)
{
    const lathist::Hist &h = ((LatHistOb *)self_)->h;
    PyObject *seq = PySequence_Fast(bounds, "bounds must be a sequence");
    if (seq == NULL)
        return NULL;
    Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    PyObject *out = PyList_New(n);
    if (out == NULL) {
        Py_DECREF(seq);
        return NULL;
    }
    for (Py_ssize_t i = 0; i < n; i++) {
        unsigned long long b = PyLong_AsUnsignedLongLong(
            PySequence_Fast_GET_ITEM(seq, i));
        if (b == (unsigned long long)-1 && PyErr_Occurred()) {
            Py_DECREF(seq);
            Py_DECREF(out);
            return NULL;
        }
        PyObject *v = PyLong_FromUnsignedLongLong(
            h.cumulative_below(lathist::index_us(b)));
        if (v == NULL) {
            Py_DECREF(seq);
            Py_DECREF(out);
            return NULL;
        }
        PyList_SET_ITEM(out, i, v);
    }
    Py_DECREF(seq);
    return out;
}

static PyObject *
LatHist_merge(PyObject *self_, PyObject *other)
{
    if (!PyObject_TypeCheck(other, &LatHistType)) {
        PyErr_SetString(PyExc_TypeError,
                        "merge() needs a native LatencyHistogram");
        return NULL;
    }
    ((LatHistOb *)self_)->h.merge(((LatHistOb *)other)->h);
    Py_RETURN_NONE;
}

static PyObject *
LatHist_reset(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    ((LatHistOb *)self_)->h.reset();
    Py_RETURN_NONE;
}

static PyObject *
lathist_ms_or_none(const lathist::Hist &h, uint64_t us)
{
    if (h.count == 0)
        Py_RETURN_NONE;
    return PyFloat_FromDouble((double)us / 1000.0);
}

static int
lathist_dict_put(PyObject *d, const char *key, PyObject *v)
{
    if (v == NULL)
        return -1;
    int r = PyDict_SetItemString(d, key, v);
    Py_DECREF(v);
    return r;
}

static PyObject *
LatHist_snapshot(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    const lathist::Hist &h = ((LatHistOb *)self_)->h;
    PyObject *d = PyDict_New();
    if (d == NULL)
        return NULL;
    if (lathist_dict_put(d, "count",
                         PyLong_FromUnsignedLongLong(h.count)) < 0 ||
        lathist_dict_put(d, "sumMs",
                         PyFloat_FromDouble((double)h.sum_us / 1000.0)) < 0 ||
        lathist_dict_put(d, "minMs", lathist_ms_or_none(h, h.min_us)) < 0 ||
        lathist_dict_put(d, "maxMs", lathist_ms_or_none(h, h.max_us)) < 0 ||
        lathist_dict_put(d, "p50", lathist_percentile(h, 0.5)) < 0 ||
        lathist_dict_put(d, "p90", lathist_percentile(h, 0.9)) < 0 ||
        lathist_dict_put(d, "p99", lathist_percentile(h, 0.99)) < 0 ||
        lathist_dict_put(d, "p999", lathist_percentile(h, 0.999)) < 0) {
        Py_DECREF(d);
        return NULL;
    }
    return d;
}

static PyObject *
LatHist_get_count(PyObject *self_, void *closure)
{
    (void)closure;
    return PyLong_FromUnsignedLongLong(((LatHistOb *)self_)->h.count);
}

static PyObject *
LatHist_get_sum_us(PyObject *self_, void *closure)
{
    (void)closure;
    return PyLong_FromUnsignedLongLong(((LatHistOb *)self_)->h.sum_us);
}

static PyObject *
LatHist_get_sum_ms(PyObject *self_, void *closure)
{
    (void)closure;
    return PyFloat_FromDouble(
        (double)((LatHistOb *)self_)->h.sum_us / 1000.0);
}

static PyObject *
LatHist_get_min_ms(PyObject *self_, void *closure)
{
    (void)closure;
    const lathist::Hist &h = ((LatHistOb *)self_)->h;
    return lathist_ms_or_none(h, h.min_us);
}

static PyObject *
LatHist_get_max_ms(PyObject *self_, void *closure)
{
    (void)closure;
    const lathist::Hist &h = ((LatHistOb *)self_)->h;
    return lathist_ms_or_none(h, h.max_us);
}

static PyMethodDef LatHist_methods[] = {
    {"record", LatHist_record, METH_O, NULL},
    {"counts", LatHist_counts, METH_NOARGS, NULL},
    {"percentile", LatHist_percentile, METH_O, NULL},
    {"cumulative", LatHist_cumulative, METH_O, NULL},
    {"merge", LatHist_merge, METH_O, NULL},
    {"reset", LatHist_reset, METH_NOARGS, NULL},
    {"snapshot", LatHist_snapshot, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

static PyGetSetDef LatHist_getset[] = {
    {(char *)"count", LatHist_get_count, NULL, NULL, NULL},
    {(char *)"sum_us", LatHist_get_sum_us, NULL, NULL, NULL},
    {(char *)"sum_ms", LatHist_get_sum_ms, NULL, NULL, NULL},
    {(char *)"min_ms", LatHist_get_min_ms, NULL, NULL, NULL},
    {(char *)"max_ms", LatHist_get_max_ms, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject LatHistType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.LatencyHistogram",
    sizeof(LatHistOb),
};

/* PoolLatency(loop, direct): the pool's wait/hold/connect histograms
 * and the clock the claim handle reads.  direct != 0 (decided once per
 * pool, only for the stock asyncio loop clock) reads CLOCK_MONOTONIC
 * in C -- the same clock time.monotonic() reads; any other loop is
 * asked through loop.time(). */
typedef struct {
    PyObject_HEAD
    PyObject *pl_loop;
    LatHistOb *pl_wait;
    LatHistOb *pl_hold;
    LatHistOb *pl_connect;
    int pl_direct;
} PoolLatOb;

extern PyTypeObject PoolLatType;
PyObject *s_p_lat;               /* "p_lat" */
extern PyObject *s_time;         /* "time" (ClaimHandleBase section) */

/* the pool clock in ms; *err set on a python failure */
static inline double
poollat_now_ms(PoolLatOb *pl, int *err)
{
#if defined(CLOCK_MONOTONIC)
    if (pl->pl_direct) {
        struct timespec ts;
        if (clock_gettime(CLOCK_MONOTONIC, &ts) == 0)
            return (double)ts.tv_sec * 1000.0 + (double)ts.tv_nsec * 1e-6;
    }
#endif
    PyObject *t = PyObject_CallMethodObjArgs(pl->pl_loop, s_time, NULL);
    if (t == NULL) {
        *err = 1;
        return 0.0;
    }
    double secs = PyFloat_AsDouble(t);
    Py_DECREF(t);
    if (secs == -1.0 && PyErr_Occurred()) {
        *err = 1;
        return 0.0;
    }
    return secs * 1000.0;
}

static PyObject *
PoolLat_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    PyObject *loop;
    int direct = 0;
    static const char *kwlist[] = {"loop", "direct", NULL};
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "O|p",
                                     const_cast<char **>(kwlist),
                                     &loop, &direct))
        return NULL;
    PoolLatOb *self = PyObject_GC_New(PoolLatOb, type);
    if (self == NULL)
        return NULL;
    Py_INCREF(loop);
    self->pl_loop = loop;
#if defined(CLOCK_MONOTONIC)
    self->pl_direct = direct;
#else
    self->pl_direct = 0;
#endif
    self->pl_wait = (LatHistOb *)LatHist_new(&LatHistType, NULL, NULL);
    self->pl_hold = (LatHistOb *)LatHist_new(&LatHistType, NULL, NULL);
    self->pl_connect = (LatHistOb *)LatHist_new(&LatHistType, NULL, NULL);
    PyObject_GC_Track((PyObject *)self);
    if (self->pl_wait == NULL || self->pl_hold == NULL ||
        self->pl_connect == NULL) {
        Py_DECREF((PyObject *)self);
        return NULL;
    }
    return (PyObject *)self;
}

static int
PoolLat_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT(((PoolLatOb *)self_)->pl_loop);
    return 0;
}

static int
PoolLat_clear_(PyObject *self_)
{
    Py_CLEAR(((PoolLatOb *)self_)->pl_loop);
    return 0;
}

static void
PoolLat_dealloc(PyObject *self_)
{
    PoolLatOb *self = (PoolLatOb *)self_;
    PyObject_GC_UnTrack(self_);
    Py_CLEAR(self->pl_loop);
    Py_CLEAR(self->pl_wait);
    Py_CLEAR(self->pl_hold);
    Py_CLEAR(self->pl_connect);
    PyObject_GC_Del(self_);
}

static PyMemberDef PoolLat_members[] = {
    {(char *)"loop", T_OBJECT, offsetof(PoolLatOb, pl_loop), READONLY,
     NULL},
    {(char *)"wait", T_OBJECT, offsetof(PoolLatOb, pl_wait), READONLY,
     NULL},
    {(char *)"hold", T_OBJECT, offsetof(PoolLatOb, pl_hold), READONLY,
     NULL},
    {(char *)"connect", T_OBJECT, offsetof(PoolLatOb, pl_connect),
     READONLY, NULL},
    {(char *)"direct", T_INT, offsetof(PoolLatOb, pl_direct), READONLY,
     NULL},
    {NULL, 0, 0, 0, NULL},
};

PyTypeObject PoolLatType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.PoolLatency",
    sizeof(PoolLatOb),
};

static void
latency_types_init(void)
{
    LatHistType.tp_flags = Py_TPFLAGS_DEFAULT;
    LatHistType.tp_methods = LatHist_methods;
    LatHistType.tp_getset = LatHist_getset;
    LatHistType.tp_new = LatHist_new;

    PoolLatType.tp_dealloc = PoolLat_dealloc;
    PoolLatType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    PoolLatType.tp_traverse = PoolLat_traverse;
    PoolLatType.tp_clear = PoolLat_clear_;
    PoolLatType.tp_members = PoolLat_members;
    PoolLatType.tp_new = PoolLat_new;
}

/* ------------------------------------------------------------------ */
/* ClaimHandleBase: the pool claim handle's hot path in C              */
/* ------------------------------------------------------------------ */

PyObject *g_err_claim_timeout;   /* errors.ClaimTimeoutError */
PyObject *g_err_cueball;         /* errors.CueballError */
PyObject *g_err_misused;         /* errors.ClaimHandleMisusedError */
PyObject *g_capture_stack;       /* utils.maybe_capture_stack_trace */

PyObject *s_claim;               /* "claim" */
PyObject *s_warn;                /* "warn" */
PyObject *s_incr;                /* "_incr_counter" */
PyObject *s_claim_timeout_evt;   /* "claim-timeout" */
PyObject *s_is_in_state;         /* "is_in_state" */
PyObject *s_time;                /* "time" */
PyObject *s_waiting, *s_claiming, *s_claimed, *s_released, *s_closed,
         *s_cancelled, *s_failed, *s_idle, *s_error_evt;
PyObject *t_waiting_valid;       /* ("claiming","cancelled","failed") */
PyObject *t_claiming_valid;      /* ("claimed","waiting","cancelled") */
PyObject *t_claimed_valid;       /* ("released","closed") */
PyObject *t_empty;               /* () */
PyObject *s_leak_events[4];      /* close, error, readable, data */

/* mirror of utils.enable/disable_stack_traces(): while capture is off
 * (the default) the shared placeholder list is used without a call */
int g_stack_on = 1;              /* until python tells us otherwise */
PyObject *g_stack_placeholder;   /* utils._DISABLED_STACK */
PyObject *g_inf;                 /* float('inf'): the no-timeout claim */

static inline PyObject *
capture_stack(void)
{
    if (!g_stack_on && g_stack_placeholder != NULL) {
        Py_INCREF(g_stack_placeholder);
        return g_stack_placeholder;
    }
    return PyObject_CallNoArgs(g_capture_stack);
}

/* defined in the SlotKit section below */
extern PyObject *s_busy_st;
/* the slot kit's preallocated conn-error callback for `handle` claimed
 * on `slot` (borrowed), or NULL if the slot has no kit */
PyObject *slotkit_conn_err_cb(PyObject *slot, PyObject *handle);

/* What the claim cycle reads of its pool on every claim and never sees
 * change: ConnectionPool.__init__ binds these attributes once and only
 * mutates the objects afterwards (docs/internals.md).  One context hangs
 * off the pool's FSMOb (f_ctx, made by pool_ctx() on the first native
 * claim or dispatch) and every handle of the pool refers to it.  It does
 * not refer to the pool.  A handle whose pool has none (not a native FSM,
 * or without these attributes), or whose log is not the pool's claim log,
 * owns a private one that holds its latency recorder and log. */
struct NQueue;
typedef struct {
    PyObject_HEAD
    struct NQueue *pc_idleq;     /* the three queues if all are the native */
    struct NQueue *pc_waiters;   /* deque, else all NULL */
    struct NQueue *pc_initq;
    PyObject *pc_counters;       /* p_counters (a dict); NULL if private */
    PyObject *pc_dead;           /* p_dead (a dict); NULL if private */
    PoolLatOb *pc_lat;           /* p_lat if it is a PoolLatency, or NULL */
    PyObject *pc_log;            /* p_claim_log, or the handle's own log */
    int pc_no_codel;             /* p_codel is None */
} PoolCtx;

extern PyTypeObject PoolCtxType;
/* the pool's context, made if need be; NULL (no error set) if `pool` is
 * not a native FSM with the attributes of a ConnectionPool.  Borrowed. */
PoolCtx *pool_ctx(PyObject *pool);
/* a handle's own context: `lat` and `log`, the queues of `base` if any */
PoolCtx *pool_ctx_private(PoolCtx *base, PoolLatOb *lat, PyObject *log);

typedef struct {
    FSMOb base;
    PyObject *chb_pool;
    PyObject *chb_claim_stack;
    PyObject *chb_callback;
    PyObject *chb_slot;
    PyObject *chb_release_stack;
    PyObject *chb_connection;
    PyObject *chb_last_error;
    PyObject *chb_waiter_node; /* ch_waiter_node: NULL or None unless
                                * the handle sits in the waiter queue */
    PoolCtx *chb_ctx;       /* owned: the pool's context or a private one
                             * (latency recorder, log, queues); NULL
                             * before _setup */
    PyObject *chb_err_conn; /* while base.f_own_reg: the connection and the */
    PyObject *chb_err_cb;   /* callback of the handle's own `error`
                             * registration, owned */
    double chb_claim_timeout;
    double chb_started;
    double chb_claimed_at;  /* valid while chb_lat_open */
    int chb_pre[4];         /* the leak detector's "before" counts */
    /* flags, one byte each (four are members, see CH_members) */
    unsigned char chb_have_pre;
    unsigned char chb_throw_error;
    unsigned char chb_cancelled;
    unsigned char chb_leak_check;
    unsigned char chb_pinger;
    unsigned char chb_lat_open;  /* wait recorded, hold still running */
    /* The library's own two listeners of a handle are not list entries.
     * The ticket: while chb_tk_on, every return to "waiting" runs the
     * pool's idle-queue handoff before any listener is called, on the
     * three queues of chb_ctx. */
    unsigned char chb_tk_on;
    unsigned char chb_tk_err_on_empty;
    /* The busy slot: armed by the slot kit's busy entry with the slot's
     * transition count at that entry (0 = not armed) and the number of
     * stateChanged listeners the handle had then.  On released/closed
     * the slot reacts after that many listeners and before the later
     * ones, and only while it still is in that same busy state. */
    unsigned long chb_bk_serial;
    Py_ssize_t chb_bk_pos;
} CHOb;

extern PyTypeObject CHType;

static inline PoolLatOb *
ch_lat(CHOb *h)
{
    return h->chb_ctx != NULL ? h->chb_ctx->pc_lat : NULL;
}

/* the handle's log (borrowed); None before _setup */
static inline PyObject *
ch_log(CHOb *h)
{
    return h->chb_ctx != NULL && h->chb_ctx->pc_log != NULL
        ? h->chb_ctx->pc_log : Py_None;
}

long
c_count_listeners(PyObject *emitter, PyObject *event)
{
    /* native-emitter path of count_listeners (callers guarantee the
     * emitter type or fall back in python) */
    if (!PyObject_TypeCheck(emitter, &EmitterType))
        return -2;  /* not ours: caller must use python fallback */
    Emitter *em = (Emitter *)emitter;
    if (em->ev_events == NULL)
        return 0;
    PyObject *ls = PyDict_GetItemWithError(em->ev_events, event);
    if (ls == NULL)
        return PyErr_Occurred() ? -1 : 0;
    long count = 0;
    Py_ssize_t n = PyList_GET_SIZE(ls);
    for (Py_ssize_t i = 0; i < n; i++) {
        PyObject *h = PyList_GET_ITEM(ls, i);
        if (!PyCallable_Check(h))
            continue;
        PyObject *marker = NULL;
        if (_PyObject_LookupAttr(h, s_internal, &marker) < 0)
            return -1;
        if (marker != NULL) {
            int truthy = PyObject_IsTrue(marker);
            Py_DECREF(marker);
            if (truthy < 0)
                return -1;
            if (truthy)
                continue;
        }
        PyObject *target = NULL;
        if (Py_TYPE(h) == &OnceWrapperType) {
            target = ((OnceWrapper *)h)->ow_listener;
            Py_INCREF(target);
        } else if (_PyObject_LookupAttr(h, s_listener, &target) < 0) {
            return -1;
        }
        if (target != NULL && target != h) {
            if (_PyObject_LookupAttr(target, s_internal, &marker) < 0) {
                Py_DECREF(target);
                return -1;
            }
            if (marker != NULL) {
                int truthy = PyObject_IsTrue(marker);
                Py_DECREF(marker);
                if (truthy < 0) {
                    Py_DECREF(target);
                    return -1;
                }
                if (truthy) {
                    Py_DECREF(target);
                    continue;
                }
            }
        }
        Py_XDECREF(target);
        count++;
    }
    return count;
}

/* The leak detector's four counts (s_leak_events order) of user
 * listeners on a connection.  Returns 0, -1 on error, or -2 when the
 * connection is not a native emitter (not ours: nothing is counted).
 * In steady state the listeners of a pooled connection are the same
 * from one claim to the next, so the counts are cached on the emitter,
 * tagged with its generation and the four list lengths (the lengths
 * catch a list changed behind the emitter's back, through _events).
 * Which lists the table holds is confirmed by the table's own version,
 * which moves when a key is added, deleted or given another value and
 * stays when a list's contents change; the cached lists are then asked
 * for their lengths.  With the tag intact this costs no lookup at all,
 * instead of a walk over every listener with two attribute lookups
 * each.  Without the version (CUEBALL_LEAK_TAG=0, or a CPython whose
 * dicts have none) the lists are looked up, four times per call. */
static inline Py_ssize_t
leak_list_len(PyObject *ls)
{
    return (ls != NULL && PyList_Check(ls)) ? PyList_GET_SIZE(ls) : -1;
}

int
emitter_leak_counts(PyObject *conn, long out[4])
{
    if (!PyObject_TypeCheck(conn, &EmitterType))
        return -2;
    Emitter *em = (Emitter *)conn;
    LeakCache *lk = em->ev_lk;
#if CUEBALL_LEAK_TAG
    if (lk != NULL && lk->lk_ok && lk->lk_gen == em->ev_gen &&
        em->ev_events != NULL &&
        lk->lk_ver == ((PyDictObject *)em->ev_events)->ma_version_tag) {
        int same = 1;
        for (int i = 0; i < 4; i++) {
            same &= (leak_list_len(lk->lk_list[i]) == lk->lk_len[i]);
        }
        if (same) {
            memcpy(out, lk->lk_cnt, sizeof(lk->lk_cnt));
            return 0;
        }
    }
#endif
    Py_ssize_t lens[4];
    PyObject *lists[4];
    uint64_t ver = 0;
#if CUEBALL_LEAK_TAG
    /* read before the lookups: a version that moves during them (a key's
     * __eq__ can run code) makes the next call look again */
    if (em->ev_events != NULL)
        ver = ((PyDictObject *)em->ev_events)->ma_version_tag;
#endif
    for (int i = 0; i < 4; i++) {
        PyObject *ls = NULL;
        if (em->ev_events != NULL) {
            ls = PyDict_GetItemWithError(em->ev_events, s_leak_events[i]);
            if (ls == NULL && PyErr_Occurred())
                return -1;
        }
        lists[i] = ls;
        lens[i] = leak_list_len(ls);
    }
    lk = em->ev_lk;
    if (lk != NULL && lk->lk_ok && lk->lk_gen == em->ev_gen &&
        memcmp(lens, lk->lk_len, sizeof(lens)) == 0 &&
        memcmp(lists, lk->lk_list, sizeof(lists)) == 0) {
        lk->lk_ver = ver;
        memcpy(out, lk->lk_cnt, sizeof(lk->lk_cnt));
        return 0;
    }
    unsigned long gen = em->ev_gen;
    for (int i = 0; i < 4; i++)
        Py_XINCREF(lists[i]);
    int failed = 0;
    for (int i = 0; i < 4 && !failed; i++) {
        long c = c_count_listeners(conn, s_leak_events[i]);
        if (c < 0)
            failed = 1;
        out[i] = c;
    }
    /* counting reads attributes of the listeners, which may run code:
     * keep the result only if no listener came or went meanwhile */
    emitter_lk_drop(em);
    lk = em->ev_lk;
    if (!failed && lk == NULL && em->ev_events != NULL) {
        lk = (LeakCache *)PyMem_Calloc(1, sizeof(LeakCache));
        em->ev_lk = lk;     /* no memory: counted again next time */
    }
    if (!failed && lk != NULL && !lk->lk_ok && gen == em->ev_gen &&
        em->ev_events != NULL) {
        memcpy(lk->lk_cnt, out, sizeof(lk->lk_cnt));
        memcpy(lk->lk_len, lens, sizeof(lens));
        for (int i = 0; i < 4; i++) {
            Py_XSETREF(lk->lk_list[i], lists[i]);
            lists[i] = NULL;
        }
        lk->lk_ver = ver;
        lk->lk_gen = gen;
        lk->lk_ok = 1;
    }
    for (int i = 0; i < 4; i++)
        Py_XDECREF(lists[i]);
    return failed ? -1 : 0;
}

/* claimed-state conn-error listener: raise if the user has no error
 * listener (and throw_error), else warn + count */
typedef struct {
    PyObject_HEAD
    PyObject *ce_handle;  /* CHOb */
} ConnErrCb;

extern PyTypeObject ConnErrCbType;

PyObject *conn_err_fire(CHOb *h, PyObject *err);

PyObject *
ConnErrCb_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    CHOb *h = (CHOb *)((ConnErrCb *)self_)->ce_handle;
    (void)kwds;
    PyObject *err = (PyTuple_GET_SIZE(args) > 0)
        ? PyTuple_GET_ITEM(args, 0) : Py_None;
    return conn_err_fire(h, err);
}

/* shared by _ConnErrCb and the slot kit's preallocated twin */
PyObject *
conn_err_fire(CHOb *h, PyObject *err)
{
    long cnt = c_count_listeners(h->chb_connection, s_error_evt);
    if (cnt == -1)
        return NULL;
    if (cnt == 0 && h->chb_throw_error) {
        /* end-user registered no 'error' listener: surface loudly
         * (lib/connection-fsm.js:697-706) */
        if (PyExceptionInstance_Check(err)) {
            PyErr_SetObject((PyObject *)Py_TYPE(err), err);
        } else {
            PyErr_SetObject(PyExc_RuntimeError, err);
        }
        return NULL;
    }
    PyObject *msg = PyUnicode_FromString(
        "connection emitted error while claimed");
    if (msg == NULL)
        return NULL;
    PyObject *r = PyObject_CallMethodObjArgs(ch_log(h), s_warn, msg,
                                             NULL);
    Py_DECREF(msg);
    if (r == NULL)
        return NULL;
    Py_DECREF(r);
    PyObject *evt = PyUnicode_FromString("error-while-claimed");
    if (evt == NULL)
        return NULL;
    r = PyObject_CallMethodObjArgs(h->chb_pool, s_incr, evt, NULL);
    Py_DECREF(evt);
    if (r == NULL)
        return NULL;
    Py_DECREF(r);
    Py_RETURN_NONE;
}

int
ConnErrCb_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT(((ConnErrCb *)self_)->ce_handle);
    return 0;
}

int
ConnErrCb_clear_(PyObject *self_)
{
    Py_CLEAR(((ConnErrCb *)self_)->ce_handle);
    return 0;
}

void
ConnErrCb_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    ConnErrCb_clear_(self_);
    PyObject_GC_Del(self_);
}

PyObject *
ConnErrCb_get_internal(PyObject *self_, void *closure)
{
    (void)self_; (void)closure;
    Py_RETURN_TRUE;   /* _cueball_internal marker */
}

PyGetSetDef ConnErrCb_getset[] = {
    {(char *)"_cueball_internal", ConnErrCb_get_internal, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject ConnErrCbType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._ConnErrCb",
    sizeof(ConnErrCb),
    0,
    ConnErrCb_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    ConnErrCb_call,
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    0,
    ConnErrCb_traverse,
    ConnErrCb_clear_,
    0, 0, 0, 0, 0, 0,
    ConnErrCb_getset,
};

/* failed-state deferred callback: cb(last_error) */
typedef struct {
    PyObject_HEAD
    PyObject *fc_handle;  /* CHOb */
} FailCb;

extern PyTypeObject FailCbType;

PyObject *
FailCb_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    CHOb *h = (CHOb *)((FailCb *)self_)->fc_handle;
    (void)args; (void)kwds;
    PyObject *err = h->chb_last_error ? h->chb_last_error : Py_None;
    return PyObject_CallOneArg(h->chb_callback, err);
}

int
FailCb_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT(((FailCb *)self_)->fc_handle);
    return 0;
}

int
FailCb_clear_(PyObject *self_)
{
    Py_CLEAR(((FailCb *)self_)->fc_handle);
    return 0;
}

void
FailCb_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    FailCb_clear_(self_);
    PyObject_GC_Del(self_);
}

PyTypeObject FailCbType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._FailCb",
    sizeof(FailCb),
    0,
    FailCb_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
    FailCb_call,
    0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC,
    0,
    FailCb_traverse,
    FailCb_clear_,
};

/* -- CH helpers ------------------------------------------------------- */

int
ch_state_is(CHOb *self, PyObject *state)
{
    return self->base.f_state == state ||
        (self->base.f_state != NULL &&
         PyUnicode_Compare(self->base.f_state, state) == 0);
}

PyObject *
ch_err_format(PyObject *cls, const char *msg)
{
    PyErr_SetString(cls, msg);
    return NULL;
}

/* -- signal methods ---------------------------------------------------- */

PyObject *
CH_try_(PyObject *self_, PyObject *slot)
{
    CHOb *self = (CHOb *)self_;
    if (!ch_state_is(self, s_waiting))
        return ch_err_format(g_fsm_error,
            "ClaimHandle.try_ only in \"waiting\"");
    PyObject *r = PyObject_CallMethodObjArgs(slot, s_is_in_state, s_idle,
                                             NULL);
    if (r == NULL)
        return NULL;
    int idle = PyObject_IsTrue(r);
    Py_DECREF(r);
    if (!idle)
        return ch_err_format(g_fsm_error,
            "ClaimHandle.try_ needs an idle slot");
    Py_INCREF(slot);
    Py_XSETREF(self->chb_slot, slot);
    if (fsm_goto_state(&self->base, s_claiming) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH_accept(PyObject *self_, PyObject *connection)
{
    CHOb *self = (CHOb *)self_;
    if (!ch_state_is(self, s_claiming))
        return ch_err_format(g_fsm_error, "accept only in claiming");
    Py_INCREF(connection);
    Py_XSETREF(self->chb_connection, connection);
    if (fsm_goto_state(&self->base, s_claimed) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH_reject(PyObject *self_, PyObject *noargs)
{
    CHOb *self = (CHOb *)self_;
    (void)noargs;
    if (!ch_state_is(self, s_claiming))
        return ch_err_format(g_fsm_error, "reject only in claiming");
    if (fsm_goto_state(&self->base,
                       self->chb_cancelled ? s_cancelled : s_waiting) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *CH_release(PyObject *self_, PyObject *noargs);

PyObject *
CH_cancel(PyObject *self_, PyObject *noargs)
{
    CHOb *self = (CHOb *)self_;
    if (ch_state_is(self, s_claimed))
        return CH_release(self_, noargs);
    self->chb_cancelled = 1;
    /* in "claiming" cancellation applies on reject/accept; in
     * "waiting" it takes effect now (lib/connection-fsm.js:580) */
    if (ch_state_is(self, s_waiting)) {
        if (fsm_goto_state(&self->base, s_cancelled) < 0)
            return NULL;
    }
    Py_RETURN_NONE;
}

int
ch_do_claim_timeout(CHOb *self)
{
    PyObject *err = PyObject_CallOneArg(g_err_claim_timeout,
                                        self->chb_pool);
    if (err == NULL)
        return -1;
    Py_XSETREF(self->chb_last_error, err);
    PyObject *r = PyObject_CallMethodObjArgs(
        self->chb_pool, s_incr, s_claim_timeout_evt, NULL);
    if (r == NULL)
        return -1;
    Py_DECREF(r);
    return fsm_goto_state(&self->base, s_failed);
}

PyObject *
CH_timeout(PyObject *self_, PyObject *noargs)
{
    CHOb *self = (CHOb *)self_;
    (void)noargs;
    if (!ch_state_is(self, s_waiting))
        return ch_err_format(g_fsm_error, "timeout only in waiting");
    if (ch_do_claim_timeout(self) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH__on_claim_timeout(PyObject *self_, PyObject *noargs)
{
    return CH_timeout(self_, noargs);
}

PyObject *
CH_fail(PyObject *self_, PyObject *err)
{
    CHOb *self = (CHOb *)self_;
    if (ch_state_is(self, s_waiting)) {
        Py_INCREF(err);
        Py_XSETREF(self->chb_last_error, err);
        if (fsm_goto_state(&self->base, s_failed) < 0)
            return NULL;
    }
    Py_RETURN_NONE;
}

int
ch_relinquish(CHOb *self, PyObject *target_state)
{
    if (!ch_state_is(self, s_claimed)) {
        if (ch_state_is(self, s_released) || ch_state_is(self, s_closed)) {
            /* capture ran from C, so the innermost python frame IS
             * the release() caller (the pure-python twin captures two
             * frames deeper and indexes -3) */
            PyObject *by = NULL;
            PyObject *stack = self->chb_release_stack;
            if (stack != NULL && PyList_Check(stack) &&
                PyList_GET_SIZE(stack) >= 1) {
                by = PyList_GET_ITEM(stack, PyList_GET_SIZE(stack) - 1);
            }
            PyObject *msg = PyUnicode_FromFormat(
                "Connection not claimed by this handle, released by %S",
                by ? by : Py_None);
            if (msg == NULL)
                return -1;
            PyObject *err = PyObject_CallOneArg(g_err_cueball, msg);
            Py_DECREF(msg);
            if (err == NULL)
                return -1;
            PyErr_SetObject(g_err_cueball, err);
            Py_DECREF(err);
            return -1;
        }
        PyObject *msg = PyUnicode_FromFormat(
            "ClaimHandle.release() called while in state \"%S\"",
            self->base.f_state ? self->base.f_state : Py_None);
        if (msg == NULL)
            return -1;
        PyErr_SetObject(g_err_cueball, msg);
        Py_DECREF(msg);
        return -1;
    }
    PyObject *stack = capture_stack();
    if (stack == NULL)
        return -1;
    Py_XSETREF(self->chb_release_stack, stack);
    return fsm_goto_state(&self->base, target_state);
}

PyObject *
CH_release(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    if (ch_relinquish((CHOb *)self_, s_released) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH_close(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    if (ch_relinquish((CHOb *)self_, s_closed) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH_disable_release_leak_check(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    ((CHOb *)self_)->chb_leak_check = 0;
    Py_RETURN_NONE;
}

/* -- state entries ------------------------------------------------------ */

PyObject *
CH_state_waiting(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    Py_INCREF(t_waiting_valid);
    Py_XSETREF(self->base.f_valid, t_waiting_valid);
    Py_CLEAR(self->chb_slot);
    self->chb_bk_serial = 0;
    if (isfinite(self->chb_claim_timeout)) {
        if (scope == NULL)
            scope = (PyObject *)fsm_need_scope(&self->base);
        if (scope == NULL)
            return NULL;
        PyObject *ms = PyFloat_FromDouble(self->chb_claim_timeout);
        if (ms == NULL)
            return NULL;
        PyObject *cb = PyObject_GetAttrString(self_, "_on_claim_timeout");
        if (cb == NULL) {
            Py_DECREF(ms);
            return NULL;
        }
        PyObject *args[2] = {ms, cb};
        PyObject *r = Scope_timeout(scope, args, 2);
        Py_DECREF(ms);
        Py_DECREF(cb);
        if (r == NULL)
            return NULL;
        Py_DECREF(r);
    }
    Py_RETURN_NONE;
}

PyObject *
CH_state_claiming(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    (void)scope;
    Py_INCREF(t_claiming_valid);
    Py_XSETREF(self->base.f_valid, t_claiming_valid);
    PyObject *slot = self->chb_slot;
    /* inline of ConnectionSlotFSM.claim() when the slot runs the
     * native busy/idle cycle (same checks, same transition) */
    if (slot != NULL && is_slot(slot) &&
        ((FSMOb *)slot)->f_fastkit != NULL) {
        FSMOb *sf = (FSMOb *)slot;
        PyObject *fs = sf->f_state;
        if (!(fs == s_idle ||
              (fs != NULL && PyUnicode_Compare(fs, s_idle) == 0))) {
            PyErr_SetString(g_fsm_error, "claim only in idle");
            return NULL;
        }
        if (slot_field_set(&((SlotOb *)slot)->sl_handle)) {
            PyErr_SetString(g_fsm_error, "slot already has a handle");
            return NULL;
        }
        slot_field_store(&((SlotOb *)slot)->sl_handle, self_);
        if (fsm_goto_state(sf, s_busy_st) < 0)
            return NULL;
        Py_RETURN_NONE;
    }
    PyObject *r = PyObject_CallMethodObjArgs(slot, s_claim,
                                             self_, NULL);
    if (r == NULL)
        return NULL;
    Py_DECREF(r);
    Py_RETURN_NONE;
}

PyObject *
CH_state_claimed(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    Py_INCREF(t_claimed_valid);
    Py_XSETREF(self->base.f_valid, t_claimed_valid);

    if (self->chb_cancelled) {
        if (fsm_goto_state(&self->base, s_released) < 0)
            return NULL;
        Py_RETURN_NONE;
    }

    PyObject *conn = self->chb_connection;
    long pre[4] = {0, 0, 0, 0};
    int lk = emitter_leak_counts(conn, pre);
    if (lk == -1)
        return NULL;
    /* listener counts: they fit an int (-2, not an emitter: zeros) */
    for (int i = 0; i < 4; i++)
        self->chb_pre[i] = lk == -2 ? 0 : (int)pre[i];
    self->chb_have_pre = 1;

    /* the slot's kit keeps one error callback for all its claims; a
     * handle claimed any other way gets one of its own */
    PyObject *ec = slotkit_conn_err_cb(self->chb_slot, self_);
    if (ec != NULL) {
        Py_INCREF(ec);
    } else {
        ConnErrCb *nec = PyObject_GC_New(ConnErrCb, &ConnErrCbType);
        if (nec == NULL)
            return NULL;
        Py_INCREF(self_);
        nec->ce_handle = self_;
        PyObject_GC_Track((PyObject *)nec);
        ec = (PyObject *)nec;
    }
    PyObject *r;
#if CUEBALL_OWN_CONN_ERR
    if (scope == NULL && !self->base.f_own_reg) {
        /* entered natively: this is the state's only registration, so
         * the handle keeps it itself and fsm_enter_loop removes it on
         * the way out, where it would dispose a scope.  Registered as
         * scope_on_c does. */
        if (Py_TYPE(conn) == &EmitterType)
            r = emitter_add((Emitter *)conn, s_error_evt, ec);
        else
            r = PyObject_CallMethodObjArgs(conn, s_on, s_error_evt, ec,
                                           NULL);
        if (r == NULL) {
            Py_DECREF(ec);
            return NULL;
        }
        Py_DECREF(r);
        Py_INCREF(conn);
        self->chb_err_conn = conn;
        self->chb_err_cb = ec;      /* our reference */
        self->base.f_own_reg = 1;
    } else
#endif
    {
        if (scope == NULL)
            scope = (PyObject *)fsm_need_scope(&self->base);
        if (scope == NULL) {
            Py_DECREF(ec);
            return NULL;
        }
        PyObject *args[3] = {conn, s_error_evt, ec};
        r = Scope_on(scope, args, 3);
        Py_DECREF(ec);
        if (r == NULL)
            return NULL;
        Py_DECREF(r);
    }

    /* the wait ends here, just before the user callback; pinger
     * claims are the pool's own and not counted */
    PoolLatOb *lat = ch_lat(self);
    if (lat != NULL && !self->chb_pinger) {
        int err = 0;
        double now = poollat_now_ms(lat, &err);
        if (err)
            return NULL;
        lat->pl_wait->h.record_ms(now - self->chb_started);
        self->chb_claimed_at = now;
        self->chb_lat_open = 1;
    }

    PyObject *cbargs[3] = {Py_None, self_, conn};
    r = PyObject_Vectorcall(self->chb_callback, cbargs, 3, NULL);
    if (r == NULL)
        return NULL;
    Py_DECREF(r);
    Py_RETURN_NONE;
}

int
ch_drop_conn_err(FSMOb *fsm)
{
    CHOb *self = (CHOb *)fsm;
    /* taken out first: removing a listener can run arbitrary code */
    PyObject *conn = self->chb_err_conn, *cb = self->chb_err_cb;
    self->chb_err_conn = self->chb_err_cb = NULL;
    fsm->f_own_reg = 0;
    if (conn == NULL || cb == NULL) {
        Py_XDECREF(conn);
        Py_XDECREF(cb);
        return 0;
    }
    /* Scope_dispose's rule: through the method if the connection's type
     * overrides remove_listener or is no native emitter */
    int rc = scope_unregister(conn, s_error_evt, cb);
    Py_DECREF(conn);
    Py_DECREF(cb);
    return rc;
}

/* claimed -> released/closed: the lease ends.  Only a handle whose
 * wait was recorded (reached its callback, not a pinger) has a hold */
static int
ch_record_hold(CHOb *self)
{
    if (!self->chb_lat_open)
        return 0;
    self->chb_lat_open = 0;
    PoolLatOb *lat = ch_lat(self);
    if (lat == NULL)
        return 0;
    int err = 0;
    double now = poollat_now_ms(lat, &err);
    if (err)
        return -1;
    lat->pl_hold->h.record_ms(now - self->chb_claimed_at);
    return 0;
}

PyObject *
CH_state_released(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    (void)scope;
    Py_INCREF(t_empty);
    Py_XSETREF(self->base.f_valid, t_empty);
    if (ch_record_hold(self) < 0)
        return NULL;
    if (!self->chb_leak_check || !self->chb_have_pre)
        Py_RETURN_NONE;
    PyObject *conn = self->chb_connection;
    /* with no listener added or removed since the "before" reading
     * this answers from the emitter's cache without a walk */
    long after[4];
    int lk = emitter_leak_counts(conn, after);
    if (lk == -1)
        return NULL;
    if (lk == -2)
        Py_RETURN_NONE;
    for (int i = 0; i < 4; i++) {
        long c = after[i];
        if (c > (long)self->chb_pre[i]) {
            PyObject *msg = PyUnicode_FromFormat(
                "connection claimer looks like it leaked event handlers "
                "(event=%S before=%ld after=%ld)",
                s_leak_events[i], (long)self->chb_pre[i], c);
            if (msg == NULL)
                return NULL;
            PyObject *r = PyObject_CallMethodObjArgs(ch_log(self), s_warn,
                                                     msg, NULL);
            Py_DECREF(msg);
            if (r == NULL)
                return NULL;
            Py_DECREF(r);
        }
    }
    Py_RETURN_NONE;
}

PyObject *
CH_state_closed(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    (void)scope;
    Py_INCREF(t_empty);
    Py_XSETREF(self->base.f_valid, t_empty);
    if (ch_record_hold(self) < 0)
        return NULL;
    Py_RETURN_NONE;
}

PyObject *
CH_state_cancelled(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    (void)scope;
    Py_INCREF(t_empty);
    Py_XSETREF(self->base.f_valid, t_empty);
    Py_RETURN_NONE;
}

PyObject *
CH_state_failed(PyObject *self_, PyObject *scope)
{
    CHOb *self = (CHOb *)self_;
    (void)scope;
    Py_INCREF(t_empty);
    Py_XSETREF(self->base.f_valid, t_empty);
    FailCb *fc = PyObject_GC_New(FailCb, &FailCbType);
    if (fc == NULL)
        return NULL;
    Py_INCREF(self_);
    fc->fc_handle = self_;
    PyObject_GC_Track((PyObject *)fc);
    /* schedule directly, not through the scope: failed is terminal so
     * the callback can never become stale, and keeping the terminal
     * scope empty lets ch_terminal_cleanup dispose it (cycle break) */
    PyObject *h = PyObject_CallMethodObjArgs(self->base.f_loop,
                                             s_call_soon,
                                             (PyObject *)fc, NULL);
    Py_DECREF(fc);
    if (h == NULL)
        return NULL;
    Py_DECREF(h);
    Py_RETURN_NONE;
}

/* -- misuse traps -------------------------------------------------------- */

PyObject *
CH_get_misused(PyObject *self_, void *closure)
{
    (void)self_; (void)closure;
    PyObject *err = PyObject_CallNoArgs(g_err_misused);
    if (err == NULL)
        return NULL;
    PyErr_SetObject(g_err_misused, err);
    Py_DECREF(err);
    return NULL;
}

PyObject *
CH_on(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs >= 1 && PyUnicode_Check(args[0])) {
        if (PyUnicode_CompareWithASCIIString(args[0], "readable") == 0 ||
            PyUnicode_CompareWithASCIIString(args[0], "close") == 0) {
            PyObject *err = PyObject_CallNoArgs(g_err_misused);
            if (err == NULL)
                return NULL;
            PyErr_SetObject(g_err_misused, err);
            Py_DECREF(err);
            return NULL;
        }
    }
    return Emitter_on(self_, args, nargs);
}

PyObject *
CH_once(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs >= 1 && PyUnicode_Check(args[0])) {
        if (PyUnicode_CompareWithASCIIString(args[0], "readable") == 0 ||
            PyUnicode_CompareWithASCIIString(args[0], "close") == 0) {
            PyObject *err = PyObject_CallNoArgs(g_err_misused);
            if (err == NULL)
                return NULL;
            PyErr_SetObject(g_err_misused, err);
            Py_DECREF(err);
            return NULL;
        }
    }
    return Emitter_once(self_, args, nargs);
}

/* Removing a listener that sits before the busy slot's place in the
 * order moves that place with it. */
PyObject *
CH_remove_listener(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    CHOb *self = (CHOb *)self_;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "remove_listener(event, listener)");
        return NULL;
    }
    Py_ssize_t at;
    if (emitter_remove_core(&self->base.base, args, &at) < 0)
        return NULL;
    if (at >= 0 && at < self->chb_bk_pos &&
        (args[0] == s_stateChanged ||
         (PyUnicode_Check(args[0]) &&
          PyUnicode_Compare(args[0], s_stateChanged) == 0)))
        self->chb_bk_pos--;
    Py_RETURN_NONE;
}

PyObject *
CH_remove_all_listeners(PyObject *self_, PyObject *const *args,
                        Py_ssize_t nargs)
{
    /* whatever is registered from here on comes after the slot */
    ((CHOb *)self_)->chb_bk_pos = 0;
    return Emitter_remove_all_listeners(self_, args, nargs);
}

/* -- init / gc ------------------------------------------------------------ */

int
CH_traverse(PyObject *self_, visitproc visit, void *arg)
{
    CHOb *self = (CHOb *)self_;
    Py_VISIT(self->chb_pool);
    Py_VISIT(self->chb_claim_stack);
    Py_VISIT(self->chb_callback);
    Py_VISIT(self->chb_slot);
    Py_VISIT(self->chb_release_stack);
    Py_VISIT(self->chb_connection);
    Py_VISIT(self->chb_last_error);
    Py_VISIT(self->chb_waiter_node);
    Py_VISIT((PyObject *)self->chb_ctx);
    Py_VISIT(self->chb_err_conn);
    Py_VISIT(self->chb_err_cb);
    return FSM_traverse(self_, visit, arg);
}

int
CH_clear_(PyObject *self_)
{
    CHOb *self = (CHOb *)self_;
    Py_CLEAR(self->chb_pool);
    Py_CLEAR(self->chb_claim_stack);
    Py_CLEAR(self->chb_callback);
    Py_CLEAR(self->chb_slot);
    Py_CLEAR(self->chb_release_stack);
    Py_CLEAR(self->chb_connection);
    Py_CLEAR(self->chb_last_error);
    Py_CLEAR(self->chb_waiter_node);
    Py_CLEAR(self->chb_ctx);
    self->base.f_own_reg = 0;
    Py_CLEAR(self->chb_err_conn);
    Py_CLEAR(self->chb_err_cb);
    return FSM_clear_(self_);
}

void
CH_dealloc(PyObject *self_)
{
    CHOb *self = (CHOb *)self_;
    PyTypeObject *tp = Py_TYPE(self_);
    PyObject_GC_UnTrack(self_);
    if (self->base.base.ev_weakrefs != NULL)
        PyObject_ClearWeakRefs(self_);
    CH_clear_(self_);
    tp->tp_free(self_);
}

/* _setup(pool, claim_stack, callback, log, claim_timeout, loop):
 * one-shot C-side initializer used by the python subclass */
PyObject *
CH__setup(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    CHOb *self = (CHOb *)self_;
    if (nargs != 7) {
        PyErr_SetString(PyExc_TypeError,
            "_setup(pool, stack, cb, log, timeout, throw_error, loop)");
        return NULL;
    }
    Py_INCREF(args[0]); Py_XSETREF(self->chb_pool, args[0]);
    Py_INCREF(args[1]); Py_XSETREF(self->chb_claim_stack, args[1]);
    Py_INCREF(args[2]); Py_XSETREF(self->chb_callback, args[2]);
    self->chb_claim_timeout = PyFloat_AsDouble(args[4]);
    if (self->chb_claim_timeout == -1.0 && PyErr_Occurred())
        return NULL;
    int throw_error = PyObject_IsTrue(args[5]);
    if (throw_error < 0)
        return NULL;
    self->chb_throw_error = throw_error;
    self->chb_cancelled = 0;
    self->chb_leak_check = 1;
    self->chb_pinger = 0;
    self->chb_have_pre = 0;
    self->chb_lat_open = 0;
    /* the pool's context holds its latency recorder (if it keeps one,
     * latencyStats), its queues and its claim log; with another log, or
     * a pool that has no context, the handle gets one of its own */
    PoolCtx *cx = pool_ctx(args[0]);
    if (cx != NULL && cx->pc_log == args[3]) {
        Py_INCREF((PyObject *)cx);
    } else {
        PyObject *lat = NULL;
        if (cx != NULL) {
            lat = (PyObject *)cx->pc_lat;
            Py_XINCREF(lat);
        } else {
            if (_PyObject_LookupAttr(args[0], s_p_lat, &lat) < 0)
                return NULL;
            if (lat != NULL && Py_TYPE(lat) != &PoolLatType)
                Py_CLEAR(lat);
        }
        cx = pool_ctx_private(cx, (PoolLatOb *)lat, args[3]);
        Py_XDECREF(lat);
        if (cx == NULL)
            return NULL;
    }
    Py_XSETREF(self->chb_ctx, cx);

    /* FSM init (resolves loop, enters "waiting") */
    PyObject *resolved = resolve_loop(args[6]);
    if (resolved == NULL)
        return NULL;
    Py_XSETREF(self->base.f_loop, resolved);
#if !CUEBALL_HANDLE_HOOKS
    /* with the hooks the event dict appears with the first on()/once() */
    if (Emitter_init(self_, NULL, NULL) < 0)
        return NULL;
#endif
    self->chb_tk_on = 0;
    self->chb_bk_serial = 0;
    if (fsm_goto_state(&self->base, s_waiting) < 0)
        return NULL;
    PoolLatOb *plat = ch_lat(self);
    if (plat != NULL && plat->pl_direct &&
        plat->pl_loop == self->base.f_loop) {
        /* stock loop clock: same reading without the python call */
        int err = 0;
        self->chb_started = poollat_now_ms(plat, &err);
        if (err)
            return NULL;
        Py_RETURN_NONE;
    }
    PyObject *t = PyObject_CallMethodObjArgs(self->base.f_loop, s_time,
                                             NULL);
    if (t == NULL)
        return NULL;
    double secs = PyFloat_AsDouble(t);
    Py_DECREF(t);
    if (secs == -1.0 && PyErr_Occurred())
        return NULL;
    self->chb_started = secs * 1000.0;
    Py_RETURN_NONE;
}

PyMethodDef CH_methods[] = {
    {"_setup", (PyCFunction)(void (*)(void))CH__setup, METH_FASTCALL, NULL},
    {"try_", CH_try_, METH_O, NULL},
    {"accept", CH_accept, METH_O, NULL},
    {"reject", CH_reject, METH_NOARGS, NULL},
    {"cancel", CH_cancel, METH_NOARGS, NULL},
    {"timeout", CH_timeout, METH_NOARGS, NULL},
    {"_on_claim_timeout", CH__on_claim_timeout, METH_NOARGS, NULL},
    {"fail", CH_fail, METH_O, NULL},
    {"release", CH_release, METH_NOARGS, NULL},
    {"close", CH_close, METH_NOARGS, NULL},
    {"disable_release_leak_check", CH_disable_release_leak_check,
     METH_NOARGS, NULL},
    {"on", (PyCFunction)(void (*)(void))CH_on, METH_FASTCALL, NULL},
    {"once", (PyCFunction)(void (*)(void))CH_once, METH_FASTCALL, NULL},
    {"remove_listener", (PyCFunction)(void (*)(void))CH_remove_listener,
     METH_FASTCALL, NULL},
    {"remove_all_listeners",
     (PyCFunction)(void (*)(void))CH_remove_all_listeners, METH_FASTCALL,
     NULL},
    {"state_waiting", CH_state_waiting, METH_O, NULL},
    {"state_claiming", CH_state_claiming, METH_O, NULL},
    {"state_claimed", CH_state_claimed, METH_O, NULL},
    {"state_released", CH_state_released, METH_O, NULL},
    {"state_closed", CH_state_closed, METH_O, NULL},
    {"state_cancelled", CH_state_cancelled, METH_O, NULL},
    {"state_failed", CH_state_failed, METH_O, NULL},
    {NULL, NULL, 0, NULL},
};

PyMemberDef CH_members[] = {
    {(char *)"ch_pool", T_OBJECT, offsetof(CHOb, chb_pool), 0, NULL},
    {(char *)"ch_claim_stack", T_OBJECT, offsetof(CHOb, chb_claim_stack),
     0, NULL},
    {(char *)"ch_callback", T_OBJECT, offsetof(CHOb, chb_callback), 0,
     NULL},
    {(char *)"ch_slot", T_OBJECT, offsetof(CHOb, chb_slot), 0, NULL},
    {(char *)"ch_release_stack", T_OBJECT,
     offsetof(CHOb, chb_release_stack), 0, NULL},
    {(char *)"ch_connection", T_OBJECT, offsetof(CHOb, chb_connection),
     0, NULL},
    {(char *)"ch_last_error", T_OBJECT, offsetof(CHOb, chb_last_error),
     0, NULL},
    {(char *)"ch_waiter_node", T_OBJECT, offsetof(CHOb, chb_waiter_node),
     0, NULL},
    {(char *)"ch_claim_timeout", T_DOUBLE,
     offsetof(CHOb, chb_claim_timeout), 0, NULL},
    {(char *)"ch_started", T_DOUBLE, offsetof(CHOb, chb_started), 0, NULL},
    {(char *)"ch_cancelled", T_UBYTE, offsetof(CHOb, chb_cancelled), 0,
     NULL},
    {(char *)"ch_throw_error", T_UBYTE, offsetof(CHOb, chb_throw_error), 0,
     NULL},
    {(char *)"ch_do_release_leak_check", T_UBYTE,
     offsetof(CHOb, chb_leak_check), 0, NULL},
    {(char *)"ch_pinger", T_UBYTE, offsetof(CHOb, chb_pinger), 0, NULL},
    {NULL, 0, 0, 0, NULL},
};

/* ch_log: the log lives in the handle's context */
PyObject *
CH_get_log(PyObject *self_, void *closure)
{
    (void)closure;
    PyObject *log = ch_log((CHOb *)self_);
    Py_INCREF(log);
    return log;
}

PyGetSetDef CH_getset[] = {
    {(char *)"ch_log", CH_get_log, NULL, NULL, NULL},
    {(char *)"readable", CH_get_misused, NULL, NULL, NULL},
    {(char *)"writable", CH_get_misused, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject CHType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.ClaimHandleBase",
    sizeof(CHOb),
    0,
    CH_dealloc,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE | Py_TPFLAGS_HAVE_GC,
    "pool claim handle (native core)",
    CH_traverse,
    CH_clear_,
    0, 0, 0, 0,
    CH_methods,
    CH_members,
    CH_getset,
    &FSMType,
    0, 0, 0,
    0,
    0,
    0,
    PyType_GenericNew,
};

/* direct dispatch of the handle's state entries (fsm_enter_loop) */
struct ChEntry {
    PyObject **ce_state;     /* interned state name */
    const char *ce_method;
    ch_entry_fn ce_fn;
    PyObject *ce_attr;       /* interned method name */
    PyObject *ce_desc;       /* CHType's own descriptor for it */
};

ChEntry ch_entries[] = {
    {&s_waiting, "state_waiting", CH_state_waiting, NULL, NULL},
    {&s_claiming, "state_claiming", CH_state_claiming, NULL, NULL},
    {&s_claimed, "state_claimed", CH_state_claimed, NULL, NULL},
    {&s_released, "state_released", CH_state_released, NULL, NULL},
    {&s_closed, "state_closed", CH_state_closed, NULL, NULL},
    {&s_cancelled, "state_cancelled", CH_state_cancelled, NULL, NULL},
    {&s_failed, "state_failed", CH_state_failed, NULL, NULL},
};
const int ch_n_entries = (int)(sizeof(ch_entries) / sizeof(ch_entries[0]));

int
ch_entries_init(void)
{
    for (int i = 0; i < ch_n_entries; i++) {
        ChEntry *e = &ch_entries[i];
        e->ce_attr = PyUnicode_InternFromString(e->ce_method);
        if (e->ce_attr == NULL)
            return -1;
        e->ce_desc = PyDict_GetItemWithError(CHType.tp_dict, e->ce_attr);
        if (e->ce_desc == NULL)
            return -1;
        Py_INCREF(e->ce_desc);
    }
    return 0;
}

ch_entry_fn
ch_direct_entry(FSMOb *self, PyObject *target)
{
    PyTypeObject *tp = Py_TYPE(self);
#if CUEBALL_EXACT_TYPES
    /* every transition of every FSM asks: the registered slot and pool
     * classes are no handles (checked when they were registered) */
    if (tp != g_handle_cls &&
        (tp == g_slot_cls || tp == g_pool_cls ||
         !PyType_IsSubtype(tp, &CHType)))
        return NULL;
#else
    if (!PyType_IsSubtype(tp, &CHType))
        return NULL;
#endif
    for (int i = 0; i < ch_n_entries; i++) {
        ChEntry *e = &ch_entries[i];
        if (*e->ce_state != target)
            continue;
        /* same test Scope_dispose applies to remove_listener: the MRO
         * still resolves the name to our own method, and (a method is
         * a non-data descriptor) the instance does not shadow it */
        if (_PyType_Lookup(tp, e->ce_attr) != e->ce_desc)
            return NULL;
        PyObject *d = self->base.ev_dict;
        if (d != NULL && PyDict_GET_SIZE(d) > 0 &&
            PyDict_GetItemWithError(d, e->ce_attr) != NULL)
            return NULL;
        if (PyErr_Occurred())
            PyErr_Clear();
        return e->ce_fn;
    }
    return NULL;
}

PyObject *
speed_set_stack_traces(PyObject *mod, PyObject *const *args,
                       Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError,
                        "_set_stack_traces(enabled, placeholder)");
        return NULL;
    }
    int on = PyObject_IsTrue(args[0]);
    if (on < 0)
        return NULL;
    g_stack_on = on;
    Py_INCREF(args[1]);
    Py_XSETREF(g_stack_placeholder, args[1]);
    Py_RETURN_NONE;
}

PyObject *
speed_set_claim_helpers(PyObject *mod, PyObject *const *args,
                        Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 4) {
        PyErr_SetString(PyExc_TypeError,
            "_set_claim_helpers(ClaimTimeoutError, CueballError, "
            "ClaimHandleMisusedError, capture_stack)");
        return NULL;
    }
    Py_INCREF(args[0]); Py_XSETREF(g_err_claim_timeout, args[0]);
    Py_INCREF(args[1]); Py_XSETREF(g_err_cueball, args[1]);
    Py_INCREF(args[2]); Py_XSETREF(g_err_misused, args[2]);
    Py_INCREF(args[3]); Py_XSETREF(g_capture_stack, args[3]);
    Py_RETURN_NONE;
}

/* ------------------------------------------------------------------ */
/* module                                                              */
/* ------------------------------------------------------------------ */

PyObject *
speed_set_helpers(PyObject *mod, PyObject *const *args, Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "_set_helpers(get_loop, FSMError)");
        return NULL;
    }
    Py_INCREF(args[0]);
    Py_XSETREF(g_get_loop, args[0]);
    Py_INCREF(args[1]);
    Py_XSETREF(g_fsm_error, args[1]);
    Py_RETURN_NONE;
}

PyObject *
speed_count_listeners(PyObject *mod, PyObject *const *args,
                      Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "count_listeners(emitter, event)");
        return NULL;
    }
    if (!PyObject_TypeCheck(args[0], &EmitterType)) {
        PyErr_SetString(PyExc_TypeError, "emitter must be an EventEmitter");
        return NULL;
    }
    Emitter *em = (Emitter *)args[0];
    if (em->ev_events == NULL)
        return PyLong_FromLong(0);
    PyObject *ls = PyDict_GetItemWithError(em->ev_events, args[1]);
    if (ls == NULL)
        return PyErr_Occurred() ? NULL : PyLong_FromLong(0);
    Py_ssize_t n = PyList_GET_SIZE(ls);
    long count = 0;
    for (Py_ssize_t i = 0; i < n; i++) {
        PyObject *h = PyList_GET_ITEM(ls, i);
        if (!PyCallable_Check(h))
            continue;
        PyObject *marker = NULL;
        if (_PyObject_LookupAttr(h, s_internal, &marker) < 0)
            return NULL;
        if (marker != NULL) {
            int truthy = PyObject_IsTrue(marker);
            Py_DECREF(marker);
            if (truthy < 0)
                return NULL;
            if (truthy)
                continue;
        }
        /* once() wrappers: look at the original listener */
        PyObject *target = NULL;
        if (Py_TYPE(h) == &OnceWrapperType) {
            target = ((OnceWrapper *)h)->ow_listener;
            Py_INCREF(target);
        } else if (_PyObject_LookupAttr(h, s_listener, &target) < 0) {
            return NULL;
        }
        if (target != NULL && target != h) {
            if (_PyObject_LookupAttr(target, s_internal, &marker) < 0) {
                Py_DECREF(target);
                return NULL;
            }
            if (marker != NULL) {
                int truthy = PyObject_IsTrue(marker);
                Py_DECREF(marker);
                if (truthy < 0) {
                    Py_DECREF(target);
                    return NULL;
                }
                if (truthy) {
                    Py_DECREF(target);
                    continue;
                }
            }
        }
        Py_XDECREF(target);
        count++;
    }
    return PyLong_FromLong(count);
}

/* ------------------------------------------------------------------ */
/* Intrusive deque (lib/queue.js): O(1) unlink by node handle.         */
/* Ownership: the list holds ONE strong ref per linked node; q_next /  */
/* q_prev / q_queue are borrowed raw pointers, valid exactly while the */
/* node is linked (q_queue != NULL).                                   */

typedef struct NQueue NQueue;

typedef struct QNode {
    PyObject_HEAD
    PyObject *value;
    struct QNode *q_next;
    struct QNode *q_prev;
    NQueue *q_queue;
} QNode;

struct NQueue {
    PyObject_HEAD
    QNode *q_first;     /* borrowed (list ref keeps it alive) */
    QNode *q_last;      /* borrowed */
    Py_ssize_t q_len;
};

extern PyTypeObject QNodeType;
extern PyTypeObject NQueueType;

static void
nqueue_unlink(NQueue *q, QNode *n)
{
    if (n->q_prev != NULL)
        n->q_prev->q_next = n->q_next;
    else
        q->q_first = n->q_next;
    if (n->q_next != NULL)
        n->q_next->q_prev = n->q_prev;
    else
        q->q_last = n->q_prev;
    n->q_next = NULL;
    n->q_prev = NULL;
    n->q_queue = NULL;
    q->q_len--;
    Py_DECREF((PyObject *)n);   /* drop the list's ref */
}

static PyObject *
QNode_remove(PyObject *self_, PyObject *noargs)
{
    QNode *n = (QNode *)self_;
    (void)noargs;
    if (n->q_queue == NULL) {
        PyErr_SetString(PyExc_ValueError,
                        "QueueNode.remove() on unlinked node");
        return NULL;
    }
    nqueue_unlink(n->q_queue, n);
    Py_RETURN_NONE;
}

static PyObject *
QNode_get_linked(PyObject *self_, void *closure)
{
    (void)closure;
    return PyBool_FromLong(((QNode *)self_)->q_queue != NULL);
}

static PyObject *
QNode_get_value(PyObject *self_, void *closure)
{
    QNode *n = (QNode *)self_;
    (void)closure;
    if (n->value == NULL)
        Py_RETURN_NONE;
    Py_INCREF(n->value);
    return n->value;
}

static int
QNode_set_value(PyObject *self_, PyObject *v, void *closure)
{
    QNode *n = (QNode *)self_;
    (void)closure;
    Py_XINCREF(v);
    Py_XSETREF(n->value, v);
    return 0;
}

static int
QNode_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT(((QNode *)self_)->value);
    return 0;
}

static int
QNode_clear_(PyObject *self_)
{
    Py_CLEAR(((QNode *)self_)->value);
    return 0;
}

static void
QNode_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    QNode_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyMethodDef QNode_methods[] = {
    {"remove", QNode_remove, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

static PyGetSetDef QNode_getset[] = {
    {"linked", QNode_get_linked, NULL, NULL, NULL},
    {"value", QNode_get_value, QNode_set_value, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject QNodeType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.QueueNode",
    sizeof(QNode),
};
/* remaining slots filled in queue_types_init() — positional
 * PyTypeObject initializers are too easy to miscount */

static QNode *
nqueue_push(NQueue *q, PyObject *value)
{
    QNode *n = PyObject_GC_New(QNode, &QNodeType);
    if (n == NULL)
        return NULL;
    Py_INCREF(value);
    n->value = value;
    n->q_next = NULL;
    n->q_prev = q->q_last;
    n->q_queue = q;
    PyObject_GC_Track((PyObject *)n);
    if (q->q_last != NULL)
        q->q_last->q_next = n;
    else
        q->q_first = n;
    q->q_last = n;
    q->q_len++;
    Py_INCREF((PyObject *)n);   /* the list's ref */
    return n;                   /* caller's ref (from New) */
}

/* Pop the first value (new ref), or NULL without error if empty. */
static PyObject *
nqueue_shift_value(NQueue *q)
{
    QNode *n = q->q_first;
    if (n == NULL)
        return NULL;
    PyObject *v = n->value;
    Py_XINCREF(v);
    Py_INCREF((PyObject *)n);   /* keep alive across unlink */
    nqueue_unlink(q, n);
    Py_DECREF((PyObject *)n);
    return v ? v : Py_NewRef(Py_None);
}

static PyObject *
NQueue_push(PyObject *self_, PyObject *value)
{
    return (PyObject *)nqueue_push((NQueue *)self_, value);
}

/* Link a new node directly behind `prev`, or at the head when `prev`
 * is NULL: the refs of nqueue_push (one for the list, one returned). */
static QNode *
nqueue_link_after(NQueue *q, QNode *prev, PyObject *value)
{
    QNode *n = PyObject_GC_New(QNode, &QNodeType);
    if (n == NULL)
        return NULL;
    QNode *nxt = prev != NULL ? prev->q_next : q->q_first;
    Py_INCREF(value);
    n->value = value;
    n->q_prev = prev;
    n->q_next = nxt;
    n->q_queue = q;
    PyObject_GC_Track((PyObject *)n);
    if (prev != NULL)
        prev->q_next = n;
    else
        q->q_first = n;
    if (nxt != NULL)
        nxt->q_prev = n;
    else
        q->q_last = n;
    q->q_len++;
    Py_INCREF((PyObject *)n);   /* the list's ref */
    return n;                   /* caller's ref (from New) */
}

static PyObject *
NQueue_unshift(PyObject *self_, PyObject *value)
{
    return (PyObject *)nqueue_link_after((NQueue *)self_, NULL, value);
}

static PyObject *
NQueue_insert_after(PyObject *self_, PyObject *const *args,
                    Py_ssize_t nargs)
{
    NQueue *q = (NQueue *)self_;
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError,
                        "Queue.insert_after(node, value)");
        return NULL;
    }
    /* q_queue is set exactly while the node is linked */
    if (!PyObject_TypeCheck(args[0], &QNodeType) ||
        ((QNode *)args[0])->q_queue != q) {
        PyErr_SetString(PyExc_ValueError,
                        "Queue.insert_after() needs a node linked in "
                        "this queue");
        return NULL;
    }
    return (PyObject *)nqueue_link_after(q, (QNode *)args[0], args[1]);
}

static PyObject *
NQueue_peek_last(PyObject *self_, PyObject *noargs)
{
    NQueue *q = (NQueue *)self_;
    (void)noargs;
    if (q->q_last == NULL) {
        PyErr_SetString(PyExc_IndexError, "peek_last from empty Queue");
        return NULL;
    }
    PyObject *v = q->q_last->value;
    if (v == NULL)
        Py_RETURN_NONE;
    Py_INCREF(v);
    return v;
}

static PyObject *
NQueue_shift(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    PyObject *v = nqueue_shift_value((NQueue *)self_);
    if (v == NULL && !PyErr_Occurred())
        PyErr_SetString(PyExc_IndexError, "shift from empty Queue");
    return v;
}

static PyObject *
NQueue_peek(PyObject *self_, PyObject *noargs)
{
    NQueue *q = (NQueue *)self_;
    (void)noargs;
    if (q->q_first == NULL) {
        PyErr_SetString(PyExc_IndexError, "peek from empty Queue");
        return NULL;
    }
    PyObject *v = q->q_first->value;
    if (v == NULL)
        Py_RETURN_NONE;
    Py_INCREF(v);
    return v;
}

static PyObject *
NQueue_is_empty(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    return PyBool_FromLong(((NQueue *)self_)->q_len == 0);
}

static PyObject *
NQueue_for_each(PyObject *self_, PyObject *cb)
{
    NQueue *q = (NQueue *)self_;
    QNode *n = q->q_first;
    Py_XINCREF((PyObject *)n);
    while (n != NULL) {
        QNode *nxt = n->q_next;
        Py_XINCREF((PyObject *)nxt);
        PyObject *args[2] = {n->value ? n->value : Py_None,
                             (PyObject *)n};
        PyObject *r = PyObject_Vectorcall(cb, args, 2, NULL);
        Py_DECREF((PyObject *)n);
        if (r == NULL) {
            Py_XDECREF((PyObject *)nxt);
            return NULL;
        }
        Py_DECREF(r);
        /* if the callback unlinked the captured successor, stop (it
         * no longer belongs to this list) — matches the pure twin's
         * generator behavior */
        if (nxt != NULL && nxt->q_queue != q) {
            Py_DECREF((PyObject *)nxt);
            break;
        }
        n = nxt;
    }
    Py_RETURN_NONE;
}

static PyObject *
NQueue_iter(PyObject *self_)
{
    /* snapshot the values; O(1)-removal users iterate rarely */
    NQueue *q = (NQueue *)self_;
    PyObject *list = PyList_New(0);
    if (list == NULL)
        return NULL;
    for (QNode *n = q->q_first; n != NULL; n = n->q_next) {
        if (PyList_Append(list, n->value ? n->value : Py_None) < 0) {
            Py_DECREF(list);
            return NULL;
        }
    }
    PyObject *it = PyObject_GetIter(list);
    Py_DECREF(list);
    return it;
}

static Py_ssize_t
NQueue_len(PyObject *self_)
{
    return ((NQueue *)self_)->q_len;
}

static PyObject *
NQueue_get_len(PyObject *self_, void *closure)
{
    (void)closure;
    return PyLong_FromSsize_t(((NQueue *)self_)->q_len);
}

static int
NQueue_traverse(PyObject *self_, visitproc visit, void *arg)
{
    NQueue *q = (NQueue *)self_;
    for (QNode *n = q->q_first; n != NULL; n = n->q_next)
        Py_VISIT((PyObject *)n);
    return 0;
}

static int
NQueue_clear_(PyObject *self_)
{
    NQueue *q = (NQueue *)self_;
    while (q->q_first != NULL) {
        QNode *n = q->q_first;
        Py_INCREF((PyObject *)n);
        nqueue_unlink(q, n);
        Py_DECREF((PyObject *)n);
    }
    return 0;
}

static void
NQueue_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    NQueue_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyObject *
NQueue_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    (void)args; (void)kwds;
    NQueue *q = PyObject_GC_New(NQueue, type);
    if (q == NULL)
        return NULL;
    q->q_first = NULL;
    q->q_last = NULL;
    q->q_len = 0;
    PyObject_GC_Track((PyObject *)q);
    return (PyObject *)q;
}

static PyMethodDef NQueue_methods[] = {
    {"push", NQueue_push, METH_O, NULL},
    {"shift", NQueue_shift, METH_NOARGS, NULL},
    {"peek", NQueue_peek, METH_NOARGS, NULL},
    {"is_empty", NQueue_is_empty, METH_NOARGS, NULL},
    {"for_each", NQueue_for_each, METH_O, NULL},
    {"unshift", NQueue_unshift, METH_O, NULL},
    {"insert_after", (PyCFunction)(void (*)(void))NQueue_insert_after,
     METH_FASTCALL, NULL},
    {"peek_last", NQueue_peek_last, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

static PyGetSetDef NQueue_getset[] = {
    {"_len", NQueue_get_len, NULL, NULL, NULL},
    {"length", NQueue_get_len, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

static PySequenceMethods NQueue_as_sequence = {
    NQueue_len,                 /* sq_length */
};

PyTypeObject NQueueType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.Queue",
    sizeof(NQueue),
};

static void
queue_types_init(void)
{
    QNodeType.tp_dealloc = QNode_dealloc;
    QNodeType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    QNodeType.tp_traverse = QNode_traverse;
    QNodeType.tp_clear = QNode_clear_;
    QNodeType.tp_methods = QNode_methods;
    QNodeType.tp_getset = QNode_getset;

    NQueueType.tp_dealloc = NQueue_dealloc;
    NQueueType.tp_as_sequence = &NQueue_as_sequence;
    NQueueType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    NQueueType.tp_traverse = NQueue_traverse;
    NQueueType.tp_clear = NQueue_clear_;
    NQueueType.tp_iter = NQueue_iter;
    NQueueType.tp_methods = NQueue_methods;
    NQueueType.tp_getset = NQueue_getset;
    NQueueType.tp_new = NQueue_new;
}

/* ------------------------------------------------------------------ */
/* ClaimTicket: the pool's per-claim driver (pool.py _ClaimTicket) in  */
/* C.  On every return of the handle to "waiting" it scans the idle    */
/* queue and performs the try_ handoff without entering Python.  On    */
/* the claim path it is no object: claim_fast switches it on as the    */
/* handle's own first hook (ch_ticket_try_next); the ClaimTicket type  */
/* is the same code as a stateChanged listener.  Anything off the hot  */
/* (pool not running, idle queue empty, errorOnEmpty) delegates to     */
/* pool._ticket_slow, which holds the full reference logic.            */

PyObject *s_running_st;      /* "running" */
PyObject *s_p_idleq_node;    /* "p_idleq_node" */
PyObject *s_p_total_conns;   /* "p_total_conns" */
PyObject *s_p_busy_hwm;      /* "p_busy_hwm" */
PyObject *s_p_demand_hwm;    /* "p_demand_hwm" */
PyObject *s_ticket_slow;     /* "_ticket_slow" */
PyObject *s_p_idleq;         /* "p_idleq" */
PyObject *s_p_waiters;       /* "p_waiters" */
PyObject *s_p_initq;         /* "p_initq" */

/* what the handoff works on: the fields of a ClaimTicket object, or a
 * view of the claim handle's own ticket fields (ch_ticket_try_next) */
typedef struct {
    PyObject *ct_pool;
    PyObject *ct_handle;     /* a CHOb */
    NQueue *ct_idleq;        /* owned; NULL => always delegate */
    NQueue *ct_waiters;      /* owned */
    NQueue *ct_initq;        /* owned */
    int ct_err_on_empty;
} TicketCore;

typedef struct {
    PyObject_HEAD
    TicketCore core;
} CTOb;

extern PyTypeObject CTType;

/* -- PoolCtx: the pool's claim context (declared with CHOb) ----------- */

PyObject *s_p_counters;          /* "p_counters" */
extern PyObject *s_p_dead;       /* "p_dead" (SlotDispatch section) */
extern PyObject *s_p_codel;      /* "p_codel" (ClaimMethod section) */
extern PyObject *s_p_claim_log;  /* "p_claim_log" */

static int
PoolCtx_traverse(PyObject *self_, visitproc visit, void *arg)
{
    PoolCtx *cx = (PoolCtx *)self_;
    Py_VISIT((PyObject *)cx->pc_idleq);
    Py_VISIT((PyObject *)cx->pc_waiters);
    Py_VISIT((PyObject *)cx->pc_initq);
    Py_VISIT(cx->pc_counters);
    Py_VISIT(cx->pc_dead);
    Py_VISIT((PyObject *)cx->pc_lat);
    Py_VISIT(cx->pc_log);
    return 0;
}

static int
PoolCtx_clear_(PyObject *self_)
{
    PoolCtx *cx = (PoolCtx *)self_;
    Py_CLEAR(cx->pc_idleq);
    Py_CLEAR(cx->pc_waiters);
    Py_CLEAR(cx->pc_initq);
    Py_CLEAR(cx->pc_counters);
    Py_CLEAR(cx->pc_dead);
    Py_CLEAR(cx->pc_lat);
    Py_CLEAR(cx->pc_log);
    return 0;
}

static void
PoolCtx_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    PoolCtx_clear_(self_);
    PyObject_GC_Del(self_);
}

PyTypeObject PoolCtxType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._PoolCtx",
    sizeof(PoolCtx),
};

static void
poolctx_type_init(void)
{
    PoolCtxType.tp_dealloc = PoolCtx_dealloc;
    PoolCtxType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    PoolCtxType.tp_traverse = PoolCtx_traverse;
    PoolCtxType.tp_clear = PoolCtx_clear_;
}

static PoolCtx *
poolctx_alloc(void)
{
    PoolCtx *cx = PyObject_GC_New(PoolCtx, &PoolCtxType);
    if (cx == NULL)
        return NULL;
    cx->pc_idleq = cx->pc_waiters = cx->pc_initq = NULL;
    cx->pc_counters = cx->pc_dead = cx->pc_log = NULL;
    cx->pc_lat = NULL;
    cx->pc_no_codel = 0;
    PyObject_GC_Track((PyObject *)cx);
    return cx;
}

PoolCtx *
pool_ctx_private(PoolCtx *base, PoolLatOb *lat, PyObject *log)
{
    PoolCtx *cx = poolctx_alloc();
    if (cx == NULL)
        return NULL;
    if (base != NULL && base->pc_idleq != NULL) {
        Py_INCREF((PyObject *)base->pc_idleq);
        cx->pc_idleq = base->pc_idleq;
        Py_INCREF((PyObject *)base->pc_waiters);
        cx->pc_waiters = base->pc_waiters;
        Py_INCREF((PyObject *)base->pc_initq);
        cx->pc_initq = base->pc_initq;
    }
    Py_XINCREF((PyObject *)lat);
    cx->pc_lat = lat;
    Py_INCREF(log);
    cx->pc_log = log;
    return cx;
}

/* Read the eight attributes once.  All must be there, with p_counters and
 * p_dead dicts: anything else is no ConnectionPool and gets no context. */
static PoolCtx *
pool_ctx_make(FSMOb *pool)
{
    PyObject *names[8] = {s_p_idleq, s_p_waiters, s_p_initq, s_p_counters,
                          s_p_dead, s_p_lat, s_p_claim_log, s_p_codel};
    PyObject *v[8] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL};
    PoolCtx *cx = NULL;
    int ok = 1;
    for (int i = 0; i < 8 && ok; i++) {
        if (_PyObject_LookupAttr((PyObject *)pool, names[i], &v[i]) < 0)
            PyErr_Clear();
        ok = v[i] != NULL;
    }
    if (ok && PyDict_Check(v[3]) && PyDict_Check(v[4]) &&
        pool->f_ctx == NULL)          /* the reads may have run code */
        cx = poolctx_alloc();
    if (cx != NULL) {
        if (PyObject_TypeCheck(v[0], &NQueueType) &&
            PyObject_TypeCheck(v[1], &NQueueType) &&
            PyObject_TypeCheck(v[2], &NQueueType)) {
            cx->pc_idleq = (NQueue *)v[0];
            cx->pc_waiters = (NQueue *)v[1];
            cx->pc_initq = (NQueue *)v[2];
            v[0] = v[1] = v[2] = NULL;
        }
        cx->pc_counters = v[3];
        cx->pc_dead = v[4];
        v[3] = v[4] = NULL;
        if (Py_TYPE(v[5]) == &PoolLatType) {
            cx->pc_lat = (PoolLatOb *)v[5];
            v[5] = NULL;
        }
        cx->pc_log = v[6];
        v[6] = NULL;
        cx->pc_no_codel = v[7] == Py_None;
        pool->f_ctx = (PyObject *)cx;
    } else if (PyErr_Occurred()) {
        PyErr_Clear();
    }
    for (int i = 0; i < 8; i++)
        Py_XDECREF(v[i]);
    return (PoolCtx *)pool->f_ctx;
}

PoolCtx *
pool_ctx(PyObject *pool)
{
    if (!is_fsm(pool))
        return NULL;
    PyObject *cx = ((FSMOb *)pool)->f_ctx;
    if (cx != NULL)
        return (PoolCtx *)cx;
    return pool_ctx_make((FSMOb *)pool);
}

/* cache the pool's queues on the ticket; a pool whose queues are not
 * the native deque leaves them NULL and the ticket permanently
 * delegates to the python slow path */
static void
ct_bind_queues(TicketCore *t, PyObject *pool)
{
    PoolCtx *cx = pool_ctx(pool);
    if (cx != NULL) {
        if (cx->pc_idleq != NULL) {
            Py_INCREF((PyObject *)cx->pc_idleq);
            t->ct_idleq = cx->pc_idleq;
            Py_INCREF((PyObject *)cx->pc_waiters);
            t->ct_waiters = cx->pc_waiters;
            Py_INCREF((PyObject *)cx->pc_initq);
            t->ct_initq = cx->pc_initq;
        }
        return;
    }
    PyObject *iq = PyObject_GetAttr(pool, s_p_idleq);
    PyObject *wq = iq ? PyObject_GetAttr(pool, s_p_waiters) : NULL;
    PyObject *nq = wq ? PyObject_GetAttr(pool, s_p_initq) : NULL;
    if (nq == NULL) {
        PyErr_Clear();
        Py_XDECREF(iq);
        Py_XDECREF(wq);
        return;
    }
    if (PyObject_TypeCheck(iq, &NQueueType) &&
        PyObject_TypeCheck(wq, &NQueueType) &&
        PyObject_TypeCheck(nq, &NQueueType)) {
        t->ct_idleq = (NQueue *)iq;
        t->ct_waiters = (NQueue *)wq;
        t->ct_initq = (NQueue *)nq;
    } else {
        Py_DECREF(iq);
        Py_DECREF(wq);
        Py_DECREF(nq);
    }
}

static int
ct_note_demand(TicketCore *t)
{
    /* O(1) inline of pool._note_demand() */
    Py_ssize_t nw = t->ct_waiters->q_len;
    Py_ssize_t ni = t->ct_initq->q_len;
    Py_ssize_t spares = t->ct_idleq->q_len + ni - nw;
    if (spares < 0)
        spares = 0;
    PyObject *tot = PyObject_GetAttr(t->ct_pool, s_p_total_conns);
    if (tot == NULL)
        return -1;
    long total = PyLong_AsLong(tot);
    Py_DECREF(tot);
    if (total == -1 && PyErr_Occurred())
        return -1;
    long busy = total - (long)spares;
    if (busy < 0)
        busy = 0;
    long extras = (long)(nw - ni);
    if (extras < 0)
        extras = 0;

    PyObject *cur = PyObject_GetAttr(t->ct_pool, s_p_busy_hwm);
    if (cur == NULL)
        return -1;
    long curv = PyLong_AsLong(cur);
    Py_DECREF(cur);
    if (curv == -1 && PyErr_Occurred())
        return -1;
    if (busy > curv) {
        PyObject *nv = PyLong_FromLong(busy);
        if (nv == NULL)
            return -1;
        int r = PyObject_SetAttr(t->ct_pool, s_p_busy_hwm, nv);
        Py_DECREF(nv);
        if (r < 0)
            return -1;
    }
    cur = PyObject_GetAttr(t->ct_pool, s_p_demand_hwm);
    if (cur == NULL)
        return -1;
    curv = PyLong_AsLong(cur);
    Py_DECREF(cur);
    if (curv == -1 && PyErr_Occurred())
        return -1;
    if (busy + extras > curv) {
        PyObject *nv = PyLong_FromLong(busy + extras);
        if (nv == NULL)
            return -1;
        int r = PyObject_SetAttr(t->ct_pool, s_p_demand_hwm, nv);
        Py_DECREF(nv);
        if (r < 0)
            return -1;
    }
    return 0;
}

PyObject *s_p_rebal_scheduled;   /* "p_rebal_scheduled" */
PyObject *s_max_claim_queue;     /* "max-claim-queue" */
PyObject *s_queued_claim;        /* "queued-claim" */
extern PyObject *s_rebalance;    /* "rebalance" (SlotDispatch section) */

/* the waiter-enqueue branch of pool._ticket_slow in C: push the
 * handle, fold the demand sample, bump the HWM/queued counters, and
 * schedule a rebalance unless one is already pending */
static int
ct_enqueue_waiter(TicketCore *t)
{
    QNode *n = nqueue_push(t->ct_waiters, t->ct_handle);
    if (n == NULL)
        return -1;
    /* the handle keeps its node so leaving 'waiting' (timeout/
     * cancel) unlinks it immediately — overload cannot accumulate
     * dead queue entries between feeds (see pool._ticket_slow) */
    Py_XSETREF(((CHOb *)t->ct_handle)->chb_waiter_node, (PyObject *)n);
    if (ct_note_demand(t) < 0)
        return -1;

    PoolCtx *cx = pool_ctx(t->ct_pool);
    PyObject *counters;
    if (cx != NULL) {
        counters = cx->pc_counters;
        Py_INCREF(counters);
    } else {
        counters = PyObject_GetAttr(t->ct_pool, s_p_counters);
    }
    if (counters == NULL)
        return -1;
    if (!PyDict_Check(counters)) {
        Py_DECREF(counters);
        PyErr_SetString(PyExc_TypeError, "p_counters must be a dict");
        return -1;
    }
    /* max-claim-queue HWM */
    PyObject *cur = PyDict_GetItemWithError(counters, s_max_claim_queue);
    if (cur == NULL && PyErr_Occurred()) {
        Py_DECREF(counters);
        return -1;
    }
    long curv = -1;
    if (cur != NULL) {
        curv = PyLong_AsLong(cur);
        if (curv == -1 && PyErr_Occurred()) {
            Py_DECREF(counters);
            return -1;
        }
    }
    if ((long)t->ct_waiters->q_len > curv) {
        PyObject *nv = PyLong_FromSsize_t(t->ct_waiters->q_len);
        if (nv == NULL || PyDict_SetItem(counters, s_max_claim_queue,
                                         nv) < 0) {
            Py_XDECREF(nv);
            Py_DECREF(counters);
            return -1;
        }
        Py_DECREF(nv);
    }
    /* queued-claim += 1 (not a tracked metric event) */
    cur = PyDict_GetItemWithError(counters, s_queued_claim);
    if (cur == NULL && PyErr_Occurred()) {
        Py_DECREF(counters);
        return -1;
    }
    long qc = 0;
    if (cur != NULL) {
        qc = PyLong_AsLong(cur);
        if (qc == -1 && PyErr_Occurred()) {
            Py_DECREF(counters);
            return -1;
        }
    }
    PyObject *nv = PyLong_FromLong(qc + 1);
    if (nv == NULL ||
        PyDict_SetItem(counters, s_queued_claim, nv) < 0) {
        Py_XDECREF(nv);
        Py_DECREF(counters);
        return -1;
    }
    Py_DECREF(nv);
    Py_DECREF(counters);

    /* rebalance() unless one is already scheduled (the common case
     * under sustained queueing) */
    PyObject *sched = PyObject_GetAttr(t->ct_pool, s_p_rebal_scheduled);
    if (sched == NULL)
        return -1;
    int pending = PyObject_IsTrue(sched);
    Py_DECREF(sched);
    if (pending < 0)
        return -1;
    if (!pending) {
        PyObject *r = PyObject_CallMethodObjArgs(t->ct_pool,
                                                 s_rebalance, NULL);
        if (r == NULL)
            return -1;
        Py_DECREF(r);
    }
    return 0;
}

static int
ct_slow(TicketCore *t)
{
    PyObject *r = PyObject_CallMethodObjArgs(
        t->ct_pool, s_ticket_slow, t->ct_handle,
        t->ct_err_on_empty ? Py_True : Py_False, NULL);
    if (r == NULL)
        return -1;
    Py_DECREF(r);
    return 0;
}

static int
ct_try_next(TicketCore *t)
{
    CHOb *h = (CHOb *)t->ct_handle;
    if (!ch_state_is(h, s_waiting))
        return 0;
    if (t->ct_idleq == NULL)
        return ct_slow(t);
    PyObject *pst = ((FSMOb *)t->ct_pool)->f_state;
    if (!(pst == s_running_st ||
          (pst != NULL && PyUnicode_Compare(pst, s_running_st) == 0)))
        return ct_slow(t);

    NQueue *q = t->ct_idleq;
    while (q->q_len > 0) {
        QNode *n = q->q_first;
        PyObject *fsm = n->value;
        Py_XINCREF(fsm);
        Py_INCREF((PyObject *)n);
        nqueue_unlink(q, n);
        Py_DECREF((PyObject *)n);
        if (fsm == NULL)
            continue;
        if (is_slot(fsm)) {
            slot_field_store(&((SlotOb *)fsm)->sl_idleq_node, Py_None);
        } else if (PyObject_SetAttr(fsm, s_p_idleq_node, Py_None) < 0) {
            Py_DECREF(fsm);
            return -1;
        }
        /* stale entries tolerated: only a slot still in 'idle' is
         * usable (lib/pool.js:934-951) */
        int isidle;
        if (is_fsm(fsm)) {
            PyObject *fs = ((FSMOb *)fsm)->f_state;
            isidle = (fs == s_idle ||
                      (fs != NULL &&
                       PyUnicode_Compare(fs, s_idle) == 0));
        } else {
            PyObject *r = PyObject_CallMethodObjArgs(
                fsm, s_is_in_state, s_idle, NULL);
            if (r == NULL) {
                Py_DECREF(fsm);
                return -1;
            }
            isidle = PyObject_IsTrue(r);
            Py_DECREF(r);
        }
        if (!isidle) {
            Py_DECREF(fsm);
            continue;
        }
        PyObject *r = CH_try_((PyObject *)h, fsm);
        Py_DECREF(fsm);
        if (r == NULL)
            return -1;
        Py_DECREF(r);
        return ct_note_demand(t);
    }
    /* idle queue empty: queue as a waiter (C) unless errorOnEmpty
     * semantics apply, which keep the full python logic */
    if (!t->ct_err_on_empty)
        return ct_enqueue_waiter(t);
    return ct_slow(t);
}

/* the handle's own ticket: same handoff, on a view of its fields */
static int
ch_ticket_try_next(CHOb *h)
{
    PoolCtx *cx = h->chb_ctx;
    if (cx == NULL)
        return 0;
    TicketCore v = {h->chb_pool, (PyObject *)h, cx->pc_idleq,
                    cx->pc_waiters, cx->pc_initq, h->chb_tk_err_on_empty};
    /* the view borrows the pool and the context with its queues */
    PyObject *pool = v.ct_pool;
    Py_INCREF(pool);
    Py_INCREF((PyObject *)cx);
    int r = ct_try_next(&v);
    Py_DECREF((PyObject *)cx);
    Py_DECREF(pool);
    return r;
}

static PyObject *
CT_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    TicketCore *t = &((CTOb *)self_)->core;
    (void)kwds;
    PyObject *st;
    if (PyTuple_GET_SIZE(args) != 1) {
        PyErr_SetString(PyExc_TypeError, "ClaimTicket(state)");
        return NULL;
    }
    st = PyTuple_GET_ITEM(args, 0);
    if (st == s_waiting ||
        (PyUnicode_Check(st) && PyUnicode_Compare(st, s_waiting) == 0)) {
        if (ct_try_next(t) < 0)
            return NULL;
    }
    Py_RETURN_NONE;
}

static int
CT_traverse(PyObject *self_, visitproc visit, void *arg)
{
    TicketCore *t = &((CTOb *)self_)->core;
    Py_VISIT(t->ct_pool);
    Py_VISIT(t->ct_handle);
    Py_VISIT((PyObject *)t->ct_idleq);
    Py_VISIT((PyObject *)t->ct_waiters);
    Py_VISIT((PyObject *)t->ct_initq);
    return 0;
}

static int
CT_clear_(PyObject *self_)
{
    TicketCore *t = &((CTOb *)self_)->core;
    Py_CLEAR(t->ct_pool);
    Py_CLEAR(t->ct_handle);
    Py_CLEAR(t->ct_idleq);
    Py_CLEAR(t->ct_waiters);
    Py_CLEAR(t->ct_initq);
    return 0;
}

static void
CT_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    CT_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyObject *
CT_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    PyObject *pool, *handle, *err_on_empty;
    (void)kwds;
    if (!PyArg_ParseTuple(args, "OOO", &pool, &handle, &err_on_empty))
        return NULL;
    if (!is_fsm(pool)) {
        PyErr_SetString(PyExc_TypeError, "pool must be a native FSM");
        return NULL;
    }
    if (!is_handle(handle)) {
        PyErr_SetString(PyExc_TypeError,
                        "handle must be a ClaimHandleBase");
        return NULL;
    }
    CTOb *tob = PyObject_GC_New(CTOb, type);
    if (tob == NULL)
        return NULL;
    TicketCore *t = &tob->core;
    Py_INCREF(pool);
    t->ct_pool = pool;
    Py_INCREF(handle);
    t->ct_handle = handle;
    t->ct_idleq = NULL;
    t->ct_waiters = NULL;
    t->ct_initq = NULL;
    t->ct_err_on_empty = PyObject_IsTrue(err_on_empty);
    PyObject_GC_Track((PyObject *)tob);
    ct_bind_queues(t, pool);
    return (PyObject *)tob;
}

PyTypeObject CTType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.ClaimTicket",
    sizeof(CTOb),
};

/* pool_claim(handle_cls, pool, cb, log, loop) -> handle | True
 * The whole no-options/no-CoDel pool.claim() body in C: bump the
 * claim counter, check the pool state (returns True when
 * stopping/stopped/failed so python builds the short-circuit error
 * without re-counting), capture the claim stack, and build
 * handle+ticket via the claim_fast core with timeout=inf. */
static PyObject *speed_claim_fast(PyObject *mod, PyObject *const *args,
                                  Py_ssize_t nargs);

static PyObject *
speed_pool_claim(PyObject *mod, PyObject *const *args, Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 5) {
        PyErr_SetString(PyExc_TypeError,
                        "pool_claim(cls, pool, cb, log, loop)");
        return NULL;
    }
    PyObject *pool = args[1];
    if (!is_fsm(pool)) {
        PyErr_SetString(PyExc_TypeError, "pool must be a native FSM");
        return NULL;
    }
    /* counters["claim"] += 1 ("claim" is not a tracked metric event) */
    PoolCtx *cx = pool_ctx(pool);
    PyObject *counters;
    if (cx != NULL) {
        counters = cx->pc_counters;
        Py_INCREF(counters);
    } else {
        counters = PyObject_GetAttr(pool, s_p_counters);
    }
    if (counters == NULL)
        return NULL;
    if (PyDict_Check(counters)) {
        PyObject *cur = PyDict_GetItemWithError(counters, s_claim);
        if (cur == NULL && PyErr_Occurred()) {
            Py_DECREF(counters);
            return NULL;
        }
        long v = 0;
        if (cur != NULL) {
            v = PyLong_AsLong(cur);
            if (v == -1 && PyErr_Occurred()) {
                Py_DECREF(counters);
                return NULL;
            }
        }
        PyObject *nv = PyLong_FromLong(v + 1);
        if (nv == NULL ||
            PyDict_SetItem(counters, s_claim, nv) < 0) {
            Py_XDECREF(nv);
            Py_DECREF(counters);
            return NULL;
        }
        Py_DECREF(nv);
    }
    Py_DECREF(counters);

    PyObject *pst = ((FSMOb *)pool)->f_state;
    int bad = 0;
    if (pst == NULL) {
        bad = 1;
    } else if (!(pst == s_running_st ||
                 PyUnicode_Compare(pst, s_running_st) == 0)) {
        /* only starting is also claim-able */
        bad = !(PyUnicode_CompareWithASCIIString(pst, "starting") == 0);
    }
    if (bad)
        Py_RETURN_TRUE;

    PyObject *stack = capture_stack();
    if (stack == NULL)
        return NULL;
    PyObject *cfargs[8] = {args[0], pool, stack, args[2], args[3],
                           g_inf, args[4], Py_False};
    PyObject *h = speed_claim_fast(NULL, cfargs, 8);
    Py_DECREF(stack);
    return h;
}

/* claim_fast(handle_cls, pool, stack, cb, log, timeout, loop,
 *            err_on_empty) -> handle
 * One C call for pool.claim's hot tail: allocate the ClaimHandle
 * subclass, run the _setup core (throw_error=True), build the native
 * ticket's queues and switch the ticket on (with CUEBALL_HANDLE_HOOKS
 * off: build a ClaimTicket and register it as stateChanged listener). */
PyObject *CH__setup(PyObject *self_, PyObject *const *args,
                    Py_ssize_t nargs);

static PyObject *
speed_claim_fast(PyObject *mod, PyObject *const *args, Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 8) {
        PyErr_SetString(PyExc_TypeError,
            "claim_fast(cls, pool, stack, cb, log, timeout, loop, "
            "err_on_empty)");
        return NULL;
    }
    PyTypeObject *cls = (PyTypeObject *)args[0];
    if (!PyType_Check(args[0]) ||
        !PyType_IsSubtype(cls, &CHType)) {
        PyErr_SetString(PyExc_TypeError,
                        "cls must be a ClaimHandleBase subclass");
        return NULL;
    }
    PyObject *pool = args[1];
    if (!is_fsm(pool)) {
        PyErr_SetString(PyExc_TypeError, "pool must be a native FSM");
        return NULL;
    }
    int err_on_empty = PyObject_IsTrue(args[7]);
    if (err_on_empty < 0)
        return NULL;

    PyObject *handle = cls->tp_alloc(cls, 0);
    if (handle == NULL)
        return NULL;
    PyObject *setup_args[7] = {pool, args[2], args[3], args[4],
                               args[5], Py_True, args[6]};
    PyObject *r = CH__setup(handle, setup_args, 7);
    if (r == NULL) {
        Py_DECREF(handle);
        return NULL;
    }
    Py_DECREF(r);

#if CUEBALL_HANDLE_HOOKS
    /* the ticket is the handle's own first hook: nothing is allocated
     * and nothing registered */
    {
        CHOb *h = (CHOb *)handle;
        if (pool_ctx(pool) == NULL) {
            /* a pool without a context: the handle's private one gets
             * whatever queues the attributes give */
            TicketCore q = {NULL, NULL, NULL, NULL, NULL, 0};
            ct_bind_queues(&q, pool);
            Py_XSETREF(h->chb_ctx->pc_idleq, q.ct_idleq);
            Py_XSETREF(h->chb_ctx->pc_waiters, q.ct_waiters);
            Py_XSETREF(h->chb_ctx->pc_initq, q.ct_initq);
        }
        h->chb_tk_err_on_empty = err_on_empty;
        h->chb_tk_on = 1;
    }
#else
    CTOb *tob = PyObject_GC_New(CTOb, &CTType);
    if (tob == NULL) {
        Py_DECREF(handle);
        return NULL;
    }
    TicketCore *t = &tob->core;
    Py_INCREF(pool);
    t->ct_pool = pool;
    Py_INCREF(handle);
    t->ct_handle = handle;
    t->ct_idleq = NULL;
    t->ct_waiters = NULL;
    t->ct_initq = NULL;
    t->ct_err_on_empty = err_on_empty;
    PyObject_GC_Track((PyObject *)tob);
    ct_bind_queues(t, pool);
    r = emitter_add((Emitter *)handle, s_stateChanged, (PyObject *)tob);
    Py_DECREF((PyObject *)tob);
    if (r == NULL) {
        Py_DECREF(handle);
        return NULL;
    }
    Py_DECREF(r);
#endif
    return handle;
}

static void
ct_type_init(void)
{
    CTType.tp_dealloc = CT_dealloc;
    CTType.tp_call = CT_call;
    CTType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    CTType.tp_traverse = CT_traverse;
    CTType.tp_clear = CT_clear_;
    CTType.tp_new = CT_new;
}

/* Terminal-state cycle breaker (see fsm_enter_loop): dispose the
 * terminal scope (fsm<->scope cycle) and retire the pool ticket (with
 * CUEBALL_HANDLE_HOOKS off: unregister it from the handle's
 * stateChanged listeners, the handle<->ticket cycle).
 * Both are semantically invisible — the terminal scope registers
 * nothing, and the ticket only reacts to 'waiting', which is
 * unreachable from a terminal state.  User listeners are untouched
 * and still receive the queued terminal stateChanged. */
void
ch_terminal_cleanup(FSMOb *self)
{
    /* unlink from the waiter queue if still queued (timeout/cancel
     * while waiting): keeps the queue free of dead entries */
    PyObject *wn = ((CHOb *)self)->chb_waiter_node;
    if (wn != NULL) {
        ((CHOb *)self)->chb_waiter_node = NULL;
        if (PyObject_TypeCheck(wn, &QNodeType) &&
            ((QNode *)wn)->q_queue != NULL)
            nqueue_unlink(((QNode *)wn)->q_queue, (QNode *)wn);
        Py_DECREF(wn);
    }
    if (self->f_scope != NULL) {
        PyObject *old = self->f_scope;
        self->f_scope = NULL;
        PyObject *r = Scope_dispose(old, NULL);
        Py_DECREF(old);
        if (r == NULL)
            PyErr_Clear();
        else
            Py_DECREF(r);
    }
#if CUEBALL_HANDLE_HOOKS
    /* "waiting" is unreachable from here: the ticket is done.  (A ticket
     * registered as a listener, _AvoidClaimTicket, removes itself.) */
    ((CHOb *)self)->chb_tk_on = 0;
#else
    Emitter *em = &self->base;
    if (em->ev_events == NULL)
        return;
    PyObject *ls = PyDict_GetItemWithError(em->ev_events, s_stateChanged);
    if (ls == NULL) {
        PyErr_Clear();
        return;
    }
    if (!PyList_Check(ls))
        return;
    for (Py_ssize_t i = PyList_GET_SIZE(ls) - 1; i >= 0; i--) {
        if (PyObject_TypeCheck(PyList_GET_ITEM(ls, i), &CTType)) {
            if (PyList_SetSlice(ls, i, i + 1, NULL) < 0) {
                PyErr_Clear();
                return;
            }
        }
    }
#endif
}

/* ------------------------------------------------------------------ */
/* SlotKit: native entries for ConnectionSlotFSM's busy/idle hot       */
/* cycle (connection_fsm.py state_busy/state_idle).  One claim/release */
/* runs idle -> busy -> idle; with the kit installed both entries and  */
/* their event reactions execute in C.  The four listeners of the two  */
/* states are not registrations: the kit notes the slot's transition   */
/* count at its busy and idle entries, and the emissions they listened */
/* to (the socket manager's and the handle's stateChanged, the slot's  */
/* own `unwanted`) call the kit while the slot still is in that very   */
/* state.  Only the claimed handle's conn-error listener is a real     */
/* registration (the leak detector and users look at that list), made  */
/* with a callback allocated once per slot.  The slot's side of a      */
/* cycle allocates nothing.  Installed only for slots without a health */
/* checker;                                                            */
/* monitor/unwanted idle entries fall back to the Python entry, and    */
/* all exit transitions out of the cycle enter Python states.          */

PyObject *s_connected_st;    /* "connected" */
PyObject *s_busy_st;         /* "busy" */
PyObject *s_stopping_st;     /* "stopping" */
PyObject *s_stopped_st;      /* "stopped" */
PyObject *s_retrying_st;     /* "retrying" */
PyObject *s_connecting_st;   /* "connecting" */
PyObject *s_killing_st;      /* "killing" */
PyObject *s_unwanted_evt;    /* "unwanted" */
PyObject *s_sm_socket;       /* "sm_socket" */
PyObject *t_busy_valid;      /* like _BUSY_VALID */
PyObject *t_idle_valid;      /* like _IDLE_VALID */

typedef struct SlotKit SlotKit;

/* preallocated listener callables; `which` selects the behavior */
enum { KCB_BUSY_SMGR = 0, KCB_BUSY_HDL, KCB_IDLE_SMGR, KCB_IDLE_UNWANTED,
       KCB_CONN_ERR, KCB_N };

typedef struct {
    PyObject_HEAD
    SlotKit *kc_kit;            /* owned */
    int kc_which;
    vectorcallfunc kc_vectorcall;
} KitCb;

struct SlotKit {
    PyObject_HEAD
    FSMOb *k_slot;              /* owned */
    PyObject *k_smgr;           /* owned; an FSMOb */
    PyObject *k_observed;       /* event-observed smgr state, owned */
    /* the slot's transition count (f_hist_n) at its last native busy
     * and idle entry: a reaction belongs to that state only while the
     * count still is what it was (0 = never entered) */
    unsigned long k_busy_serial;
    unsigned long k_idle_serial;
    PyObject *k_cbs[KCB_N];        /* owned KitCb instances */
};

extern PyTypeObject SlotKitType;
extern PyTypeObject KitCbType;

PyObject *
slotkit_conn_err_cb(PyObject *slot, PyObject *handle)
{
    if (slot == NULL || !is_slot(slot))
        return NULL;
    PyObject *kit = ((FSMOb *)slot)->f_fastkit;
    if (kit == NULL || Py_TYPE(kit) != &SlotKitType ||
        ((SlotKit *)kit)->k_slot != (FSMOb *)slot ||
        ((SlotOb *)slot)->sl_handle != handle)
        return NULL;
    return ((SlotKit *)kit)->k_cbs[KCB_CONN_ERR];
}

static int
kit_goto(SlotKit *k, unsigned long serial, PyObject *state)
{
    if (serial == 0 || k->k_slot->f_hist_n != serial)
        return 0;  /* stale handler in the same cascade: obsolete */
    return fsm_goto_state(k->k_slot, state);
}

static int
kit_busy_on_release(SlotKit *k)
{
    unsigned long S = k->k_busy_serial;
    PyObject *st = k->k_observed;
    int wanted = slot_field_true(&((SlotOb *)k->k_slot)->sl_wanted);
    if (wanted < 0)
        return -1;
    if (st == s_connected_st ||
        (st != NULL && PyUnicode_Compare(st, s_connected_st) == 0))
        return kit_goto(k, S, wanted ? s_idle : s_stopping_st);
    if (st == s_closed || PyUnicode_Compare(st, s_closed) == 0)
        return kit_goto(k, S, wanted ? s_connecting_st : s_stopped_st);
    if (st == s_error_evt || PyUnicode_Compare(st, s_error_evt) == 0)
        return kit_goto(k, S, s_retrying_st);
    PyErr_Format(g_fsm_error,
                 "Handle released while smgr was in unhandled state %R",
                 st ? st : Py_None);
    return -1;
}

static int
kit_busy_on_close(SlotKit *k)
{
    unsigned long S = k->k_busy_serial;
    PyObject *st = k->k_observed;
    if (st == s_connected_st ||
        (st != NULL && PyUnicode_Compare(st, s_connected_st) == 0))
        return kit_goto(k, S, s_killing_st);
    return kit_goto(k, S, s_retrying_st);
}

static int
kit_idle_smgr_changed(SlotKit *k, PyObject *st)
{
    unsigned long S = k->k_idle_serial;
    int wanted = slot_field_true(&((SlotOb *)k->k_slot)->sl_wanted);
    if (wanted < 0)
        return -1;
    if (st == s_error_evt || PyUnicode_Compare(st, s_error_evt) == 0)
        return kit_goto(k, S, wanted ? s_retrying_st : s_stopped_st);
    if (st == s_closed || PyUnicode_Compare(st, s_closed) == 0)
        return kit_goto(k, S, wanted ? s_connecting_st : s_stopped_st);
    PyErr_Format(g_fsm_error,
                 "Unhandled smgr state transition: connected => %R", st);
    return -1;
}

static int
kit_idle_unwanted(SlotKit *k)
{
    /* mirror of _idle_on_unwanted incl. the same-spin death fix */
    unsigned long S = k->k_idle_serial;
    PyObject *sst = ((FSMOb *)k->k_smgr)->f_state;
    if (sst == s_connected_st ||
        (sst != NULL && PyUnicode_Compare(sst, s_connected_st) == 0))
        return kit_goto(k, S, s_stopping_st);
    if (sst == s_error_evt || sst == s_closed ||
        (sst != NULL && (PyUnicode_Compare(sst, s_error_evt) == 0 ||
                         PyUnicode_Compare(sst, s_closed) == 0)))
        return kit_goto(k, S, s_stopped_st);
    return 0;
}

static PyObject *
kitcb_fire(PyObject *self_, PyObject *st)
{
    KitCb *cb = (KitCb *)self_;
    SlotKit *k = cb->kc_kit;
    int r = 0;
    switch (cb->kc_which) {
    case KCB_BUSY_SMGR:
        /* record the smgr state as observed through events
         * (lib/connection-fsm.js:885-890) */
        if (st != NULL) {
            Py_INCREF(st);
            Py_XSETREF(k->k_observed, st);
        }
        break;
    case KCB_BUSY_HDL:
        if (st == s_released ||
            (st != NULL && PyUnicode_Compare(st, s_released) == 0))
            r = kit_busy_on_release(k);
        else if (st == s_closed ||
                 (st != NULL && PyUnicode_Compare(st, s_closed) == 0))
            r = kit_busy_on_close(k);
        break;
    case KCB_IDLE_SMGR:
        r = kit_idle_smgr_changed(k, st);
        break;
    case KCB_IDLE_UNWANTED:
        r = kit_idle_unwanted(k);
        break;
    case KCB_CONN_ERR: {
        /* registered by the claimed state of the slot's current handle
         * and removed when that state is left, so the handle is the
         * slot's */
        PyObject *hdl = ((SlotOb *)k->k_slot)->sl_handle;
        if (hdl == NULL || !is_handle(hdl))
            break;
        Py_INCREF(hdl);
        PyObject *res = conn_err_fire((CHOb *)hdl,
                                      st != NULL ? st : Py_None);
        Py_DECREF(hdl);
        return res;
    }
    }
    if (r < 0)
        return NULL;
    Py_RETURN_NONE;
}

static PyObject *
KitCb_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    (void)kwds;
    return kitcb_fire(self_, PyTuple_GET_SIZE(args) >= 1
                      ? PyTuple_GET_ITEM(args, 0) : NULL);
}

static PyObject *
KitCb_vectorcall(PyObject *self_, PyObject *const *args, size_t nargsf,
                 PyObject *kwnames)
{
    (void)kwnames;
    return kitcb_fire(self_, PyVectorcall_NARGS(nargsf) >= 1 ? args[0]
                                                             : NULL);
}

static int
KitCb_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT((PyObject *)((KitCb *)self_)->kc_kit);
    return 0;
}

static int
KitCb_clear_(PyObject *self_)
{
    Py_CLEAR(((KitCb *)self_)->kc_kit);
    return 0;
}

static void
KitCb_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    KitCb_clear_(self_);
    PyObject_GC_Del(self_);
}

PyTypeObject KitCbType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._SlotKitCb",
    sizeof(KitCb),
};

/* -- the native state entries --------------------------------------- */

static int
kit_state_busy(SlotKit *k)
{
    FSMOb *slot = k->k_slot;
    Py_INCREF(t_busy_valid);
    Py_XSETREF(slot->f_valid, t_busy_valid);

    PyObject *hdl = ((SlotOb *)slot)->sl_handle;
    if (hdl == NULL)
        hdl = Py_None;
    Py_INCREF(hdl);
    Py_INCREF(s_connected_st);
    Py_XSETREF(k->k_observed, s_connected_st);
    k->k_busy_serial = slot->f_hist_n;

#if !CUEBALL_SLOT_HOOKS
    {
        Scope *scope = fsm_need_scope(slot);
        if (scope == NULL ||
            scope_on_c(scope, k->k_smgr, s_stateChanged,
                       k->k_cbs[KCB_BUSY_SMGR]) < 0) {
            Py_DECREF(hdl);
            return -1;
        }
    }
#endif
    int armed = 0;
#if CUEBALL_HANDLE_HOOKS
    if (is_handle(hdl)) {
        /* the handle calls back by itself (ch_slot_hook), in the place
         * a listener registered now would have */
        CHOb *h = (CHOb *)hdl;
        PyObject *ls = h->base.base.ev_events == NULL ? NULL :
            PyDict_GetItemWithError(h->base.base.ev_events, s_stateChanged);
        if (ls == NULL && PyErr_Occurred()) {
            Py_DECREF(hdl);
            return -1;
        }
        h->chb_bk_pos = (ls != NULL && PyList_Check(ls))
            ? PyList_GET_SIZE(ls) : 0;
        h->chb_bk_serial = k->k_busy_serial;
        armed = 1;
    }
#endif
    if (!armed) {
        Scope *scope = fsm_need_scope(slot);
        if (scope == NULL ||
            scope_on_c(scope, hdl, s_stateChanged,
                       k->k_cbs[KCB_BUSY_HDL]) < 0) {
            Py_DECREF(hdl);
            return -1;
        }
    }

    PyObject *sst = ((FSMOb *)k->k_smgr)->f_state;
    int connected = (sst == s_connected_st ||
                     (sst != NULL &&
                      PyUnicode_Compare(sst, s_connected_st) == 0));
    PyObject *r;
    if (connected) {
        PyObject *sock = PyObject_GetAttr(k->k_smgr, s_sm_socket);
        if (sock == NULL) {
            Py_DECREF(hdl);
            return -1;
        }
        r = CH_accept(hdl, sock);
        Py_DECREF(sock);
        Py_DECREF(hdl);
        if (r == NULL)
            return -1;
        Py_DECREF(r);
    } else {
        /* lost the race with the smgr: treat as released
         * (lib/connection-fsm.js:1129-1196) */
        r = CH_reject(hdl, NULL);
        Py_DECREF(hdl);
        if (r == NULL)
            return -1;
        Py_DECREF(r);
        slot_field_store(&((SlotOb *)slot)->sl_handle, Py_None);
        if (kit_busy_on_release(k) < 0)
            return -1;
    }
    return 1;
}

static int
kit_state_idle(SlotKit *k)
{
    FSMOb *slot = k->k_slot;
    /* the monitor-conversion and unwanted cases keep the full Python
     * entry (cold paths with documented divergences) */
    int monitor = slot_field_true(&((SlotOb *)slot)->sl_monitor);
    if (monitor < 0)
        return -1;
    if (monitor)
        return 0;
    int wanted = slot_field_true(&((SlotOb *)slot)->sl_wanted);
    if (wanted < 0)
        return -1;
    if (!wanted)
        return 0;

    Py_INCREF(t_idle_valid);
    Py_XSETREF(slot->f_valid, t_idle_valid);
    k->k_idle_serial = slot->f_hist_n;

    SlotOb *so = (SlotOb *)slot;
    if (slot_field_set(&so->sl_handle)) {
        /* csf_prev_handle = csf_handle; csf_handle = None.  The old
         * previous handle is let go last: freeing it can run code */
        PyObject *old_prev = so->sl_prev_handle;
        so->sl_prev_handle = so->sl_handle;
        Py_INCREF(Py_None);
        so->sl_handle = Py_None;
        Py_XDECREF(old_prev);
    }

#if !CUEBALL_SLOT_HOOKS
    Scope *scope = fsm_need_scope(slot);
    if (scope == NULL)
        return -1;
    if (scope_on_c(scope, k->k_smgr, s_stateChanged,
                   k->k_cbs[KCB_IDLE_SMGR]) < 0)
        return -1;
    if (scope_on_c(scope, (PyObject *)slot, s_unwanted_evt,
                   k->k_cbs[KCB_IDLE_UNWANTED]) < 0)
        return -1;
#endif
    return 1;
}

int
slotkit_maybe_entry(PyObject *kit_, FSMOb *fsm, PyObject *target)
{
    SlotKit *k = (SlotKit *)kit_;
    if (k->k_slot != fsm)
        return 0;
    if (target == s_busy_st ||
        (PyUnicode_Check(target) &&
         PyUnicode_Compare(target, s_busy_st) == 0))
        return kit_state_busy(k);
    if (target == s_idle ||
        (PyUnicode_Check(target) &&
         PyUnicode_Compare(target, s_idle) == 0))
        return kit_state_idle(k);
    return 0;
}

/* -- the hooks: what the kit's four listeners did, called by the ------ */
/* -- emissions themselves -------------------------------------------- */

static inline int
str_is(PyObject *a, PyObject *b)
{
    return a == b || (a != NULL && PyUnicode_Check(a) &&
                      PyUnicode_Compare(a, b) == 0);
}

/* stateChanged of the socket manager, after the listeners in its list
 * (where the per-entry registration, always the newest, used to sit) */
unsigned long
slotkit_slot_serial(PyObject *kit_)
{
    SlotKit *k = (SlotKit *)kit_;
    if (Py_TYPE(kit_) != &SlotKitType || k->k_slot == NULL)
        return 0;
    return k->k_slot->f_hist_n;
}

int
slotkit_smgr_hook(PyObject *kit_, PyObject *st, unsigned long serial)
{
#if CUEBALL_SLOT_HOOKS
    SlotKit *k = (SlotKit *)kit_;
    if (Py_TYPE(kit_) != &SlotKitType || k->k_slot == NULL)
        return 0;
    unsigned long now = k->k_slot->f_hist_n;
    if (now == 0 || now != serial)
        return 0;       /* the slot moved while the listeners ran */
    if (now == k->k_busy_serial) {
        /* record the smgr state as observed through events
         * (lib/connection-fsm.js:885-890) */
        Py_INCREF(st);
        Py_XSETREF(k->k_observed, st);
        return 0;
    }
    if (now == k->k_idle_serial) {
        Py_INCREF(kit_);
        int r = kit_idle_smgr_changed(k, st);
        Py_DECREF(kit_);
        return r;
    }
#else
    (void)kit_; (void)st;
#endif
    return 0;
}

/* released/closed of a handle whose slot is in the busy state that armed
 * it: the slot moves on.  Anything else: nothing. */
static int
ch_slot_hook(CHOb *h, PyObject *st)
{
    PyObject *slot = h->chb_slot;
    if (h->chb_bk_serial == 0 || slot == NULL ||
        !is_slot(slot))
        return 0;
    PyObject *kit_ = ((FSMOb *)slot)->f_fastkit;
    if (kit_ == NULL || Py_TYPE(kit_) != &SlotKitType)
        return 0;
    SlotKit *k = (SlotKit *)kit_;
    if (k->k_slot != (FSMOb *)slot ||
        k->k_busy_serial != h->chb_bk_serial ||
        k->k_slot->f_hist_n != h->chb_bk_serial)
        return 0;       /* the slot has left that busy state: stale */
    int r = 0;
    Py_INCREF(kit_);
    if (str_is(st, s_released))
        r = kit_busy_on_release(k);
    else if (str_is(st, s_closed))
        r = kit_busy_on_close(k);
    Py_DECREF(kit_);
    return r;
}

/* One stateChanged of a claim handle.  Order: the ticket (it used to be
 * the first listener), the listeners registered before the slot went
 * busy, the slot, the listeners registered after. */
int
ch_emit_state_changed(FSMOb *self, PyObject *st)
{
    CHOb *h = (CHOb *)self;
    /* the listeners of this emission are those there are now: one added
     * while the ticket or the slot runs (in the claim callback, say)
     * first hears of the next state */
    PyObject *ls = NULL;
    if (self->base.ev_events != NULL) {
        ls = PyDict_GetItemWithError(self->base.ev_events, s_stateChanged);
        if (ls == NULL && PyErr_Occurred())
            return -1;
    }
    Py_ssize_t n = ls != NULL ? PyList_GET_SIZE(ls) : 0;
    int hook = h->chb_bk_serial != 0 &&
        (str_is(st, s_released) || str_is(st, s_closed));
    Py_ssize_t pos = !hook ? -1 : h->chb_bk_pos < n ? h->chb_bk_pos : n;
    PyObject *snap = NULL;
    if (n > 0) {
        snap = PyList_GetSlice(ls, 0, n);
        if (snap == NULL)
            return -1;
    }
    if (h->chb_tk_on && str_is(st, s_waiting)) {
        if (ch_ticket_try_next(h) < 0) {
            Py_XDECREF(snap);
            return -1;
        }
    }
    if (n == 0)
        return hook ? ch_slot_hook(h, st) : 0;
    for (Py_ssize_t i = 0; i <= n; i++) {
        if (i == pos && ch_slot_hook(h, st) < 0) {
            Py_DECREF(snap);
            return -1;
        }
        if (i == n)
            break;
        PyObject *r = PyObject_Vectorcall(PyList_GET_ITEM(snap, i), &st, 1,
                                          NULL);
        if (r == NULL) {
            Py_DECREF(snap);
            return -1;
        }
        Py_DECREF(r);
    }
    Py_DECREF(snap);
    return 1;
}

/* slot.emit(): `unwanted` reaches the kit after the listeners in the
 * list, while the slot is in the idle state the kit entered */
static PyObject *
Slot_emit(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs < 1) {
        PyErr_SetString(PyExc_TypeError, "emit(event, *args)");
        return NULL;
    }
    FSMOb *slot = (FSMOb *)self_;
    unsigned long serial = slot->f_hist_n;
    int r = emitter_emit_core((Emitter *)self_, args[0], args + 1,
                              nargs - 1);
    if (r < 0)
        return NULL;
#if CUEBALL_SLOT_HOOKS
    PyObject *kit_ = slot->f_fastkit;
    if (kit_ != NULL && Py_TYPE(kit_) == &SlotKitType &&
        str_is(args[0], s_unwanted_evt)) {
        SlotKit *k = (SlotKit *)kit_;
        if (k->k_slot == slot && serial != 0 &&
            slot->f_hist_n == serial && serial == k->k_idle_serial) {
            Py_INCREF(kit_);
            int hr = kit_idle_unwanted(k);
            Py_DECREF(kit_);
            if (hr < 0)
                return NULL;
            r = 1;
        }
    }
#endif
    return PyBool_FromLong(r);
}

/* an idle slot listens for `unwanted`, registration or not */
static PyObject *
Slot_event_names(PyObject *self_, PyObject *noargs)
{
    PyObject *names = Emitter_event_names(self_, noargs);
#if CUEBALL_SLOT_HOOKS
    if (names == NULL)
        return NULL;
    FSMOb *slot = (FSMOb *)self_;
    PyObject *kit_ = slot->f_fastkit;
    if (kit_ != NULL && Py_TYPE(kit_) == &SlotKitType &&
        ((SlotKit *)kit_)->k_slot == slot && slot->f_hist_n != 0 &&
        slot->f_hist_n == ((SlotKit *)kit_)->k_idle_serial) {
        int has = PySequence_Contains(names, s_unwanted_evt);
        if (has < 0 || (!has && PyList_Append(names, s_unwanted_evt) < 0)) {
            Py_DECREF(names);
            return NULL;
        }
    }
#endif
    return names;
}

static PyMethodDef Slot_methods[] = {
    {"emit", (PyCFunction)(void (*)(void))Slot_emit, METH_FASTCALL, NULL},
    {"event_names", Slot_event_names, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

/* ------------------------------------------------------------------ */
/* ControlledDelay: the CoDel AQM (codel.py / lib/codel.js) in C so    */
/* the overload-shed feed path stays native.                           */

#define CODEL_INTERVAL_MS 100.0

typedef struct {
    PyObject_HEAD
    PyObject *cd_loop;          /* owned */
    double cd_targdelay;
    double cd_first_above_time;
    double cd_drop_next;
    long cd_count;
    int cd_dropping;
    double cd_last_empty;
} CoDelOb;

extern PyTypeObject CoDelType;

static double
codel_now(CoDelOb *self, int *err)
{
    PyObject *t = PyObject_CallMethodObjArgs(self->cd_loop, s_time, NULL);
    if (t == NULL) {
        *err = 1;
        return 0.0;
    }
    double secs = PyFloat_AsDouble(t);
    Py_DECREF(t);
    if (secs == -1.0 && PyErr_Occurred()) {
        *err = 1;
        return 0.0;
    }
    *err = 0;
    return secs * 1000.0;
}

static int
codel_can_drop(CoDelOb *self, double now, double start)
{
    double sojourn = now - start;
    if (sojourn < self->cd_targdelay)
        self->cd_first_above_time = 0.0;
    else if (self->cd_first_above_time == 0.0)
        self->cd_first_above_time = now + CODEL_INTERVAL_MS;
    else if (now >= self->cd_first_above_time)
        return 1;
    return 0;
}

/* int result: 1 drop, 0 keep, -1 error.  Mirrors
 * ControlledDelay.overloaded() exactly. */
static int
codel_overloaded_c(CoDelOb *self, double start)
{
    int err = 0;
    double now = codel_now(self, &err);
    if (err)
        return -1;
    int ok_to_drop = codel_can_drop(self, now, start);
    int drop_claim = 0;
    if (self->cd_dropping) {
        if (!ok_to_drop) {
            self->cd_dropping = 0;
        } else if (now >= self->cd_drop_next) {
            /* NOTE: the reference deliberately does NOT advance
             * cd_drop_next here (lib/codel.js:62-68): once dropping
             * and past drop-next, every dequeue above target drops
             * until the sojourn falls below target again. */
            drop_claim = 1;
            self->cd_count++;
        }
    } else if (ok_to_drop &&
               ((now - self->cd_drop_next < CODEL_INTERVAL_MS) ||
                (now - self->cd_first_above_time >=
                 CODEL_INTERVAL_MS))) {
        drop_claim = 1;
        self->cd_dropping = 1;
        if (now - self->cd_drop_next < CODEL_INTERVAL_MS)
            self->cd_count = self->cd_count > 2 ?
                self->cd_count - 2 : 1;
        else
            self->cd_count = 1;
        self->cd_drop_next = now +
            CODEL_INTERVAL_MS / sqrt((double)self->cd_count);
    }
    return drop_claim;
}

static PyObject *
CoDel_overloaded(PyObject *self_, PyObject *start_)
{
    double start = PyFloat_AsDouble(start_);
    if (start == -1.0 && PyErr_Occurred())
        return NULL;
    int r = codel_overloaded_c((CoDelOb *)self_, start);
    if (r < 0)
        return NULL;
    return PyBool_FromLong(r);
}

static PyObject *
CoDel_can_drop(PyObject *self_, PyObject *const *args, Py_ssize_t nargs)
{
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "can_drop(now, start)");
        return NULL;
    }
    double now = PyFloat_AsDouble(args[0]);
    if (now == -1.0 && PyErr_Occurred())
        return NULL;
    double start = PyFloat_AsDouble(args[1]);
    if (start == -1.0 && PyErr_Occurred())
        return NULL;
    return PyBool_FromLong(codel_can_drop((CoDelOb *)self_, now, start));
}

static PyObject *
CoDel_get_drop_next(PyObject *self_, PyObject *now_)
{
    CoDelOb *self = (CoDelOb *)self_;
    double now = PyFloat_AsDouble(now_);
    if (now == -1.0 && PyErr_Occurred())
        return NULL;
    return PyFloat_FromDouble(
        now + CODEL_INTERVAL_MS / sqrt((double)self->cd_count));
}

static int
codel_empty_c(CoDelOb *self)
{
    int err = 0;
    double now = codel_now(self, &err);
    if (err)
        return -1;
    self->cd_last_empty = now;
    self->cd_first_above_time = 0.0;
    return 0;
}

static PyObject *
CoDel_empty(PyObject *self_, PyObject *noargs)
{
    (void)noargs;
    if (codel_empty_c((CoDelOb *)self_) < 0)
        return NULL;
    Py_RETURN_NONE;
}

static PyObject *
CoDel_get_max_idle(PyObject *self_, PyObject *noargs)
{
    CoDelOb *self = (CoDelOb *)self_;
    (void)noargs;
    double bound = self->cd_targdelay * 10.0;
    int err = 0;
    double now = codel_now(self, &err);
    if (err)
        return NULL;
    if (self->cd_last_empty < now - bound)
        return PyFloat_FromDouble(self->cd_targdelay * 3.0);
    return PyFloat_FromDouble(bound);
}

static PyObject *
CoDel_get_dropping(PyObject *self_, void *closure)
{
    (void)closure;
    return PyBool_FromLong(((CoDelOb *)self_)->cd_dropping);
}

static int
CoDel_traverse(PyObject *self_, visitproc visit, void *arg)
{
    Py_VISIT(((CoDelOb *)self_)->cd_loop);
    return 0;
}

static int
CoDel_clear_(PyObject *self_)
{
    Py_CLEAR(((CoDelOb *)self_)->cd_loop);
    return 0;
}

static void
CoDel_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    CoDel_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyObject *
CoDel_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    PyObject *target, *loop = Py_None;
    static const char *kwlist[] = {"target_claim_delay", "loop", NULL};
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "O|O",
                                     const_cast<char **>(kwlist),
                                     &target, &loop))
        return NULL;
    double targ;
    if (PyFloat_Check(target) || PyLong_Check(target)) {
        targ = PyFloat_AsDouble(target);
        if (targ == -1.0 && PyErr_Occurred())
            return NULL;
    } else {
        PyErr_SetString(PyExc_ValueError,
                        "target_claim_delay must be finite");
        return NULL;
    }
    if (!std::isfinite(targ)) {
        PyErr_SetString(PyExc_ValueError,
                        "target_claim_delay must be finite");
        return NULL;
    }
    PyObject *resolved = PyObject_CallOneArg(g_get_loop, loop);
    if (resolved == NULL)
        return NULL;
    CoDelOb *self = PyObject_GC_New(CoDelOb, type);
    if (self == NULL) {
        Py_DECREF(resolved);
        return NULL;
    }
    self->cd_loop = resolved;
    self->cd_targdelay = targ;
    self->cd_first_above_time = 0.0;
    self->cd_drop_next = 0.0;
    self->cd_count = 0;
    self->cd_dropping = 0;
    self->cd_last_empty = 0.0;
    PyObject_GC_Track((PyObject *)self);
    /* treat the queue as having just been empty (see codel.py) */
    int err = 0;
    double now = codel_now(self, &err);
    if (err) {
        Py_DECREF((PyObject *)self);
        return NULL;
    }
    self->cd_last_empty = now;
    return (PyObject *)self;
}

static PyMethodDef CoDel_methods[] = {
    {"overloaded", CoDel_overloaded, METH_O, NULL},
    {"can_drop", (PyCFunction)(void (*)(void))CoDel_can_drop,
     METH_FASTCALL, NULL},
    {"get_drop_next", CoDel_get_drop_next, METH_O, NULL},
    {"empty", CoDel_empty, METH_NOARGS, NULL},
    {"get_max_idle", CoDel_get_max_idle, METH_NOARGS, NULL},
    {NULL, NULL, 0, NULL},
};

static PyMemberDef CoDel_members[] = {
    {(char *)"cd_targdelay", T_DOUBLE, offsetof(CoDelOb, cd_targdelay),
     READONLY, NULL},
    {(char *)"cd_first_above_time", T_DOUBLE,
     offsetof(CoDelOb, cd_first_above_time), 0, NULL},
    {(char *)"cd_drop_next", T_DOUBLE, offsetof(CoDelOb, cd_drop_next),
     0, NULL},
    {(char *)"cd_count", T_LONG, offsetof(CoDelOb, cd_count), 0, NULL},
    {(char *)"cd_last_empty", T_DOUBLE,
     offsetof(CoDelOb, cd_last_empty), 0, NULL},
    {NULL, 0, 0, 0, NULL},
};

static PyGetSetDef CoDel_getset[] = {
    {(char *)"cd_dropping", CoDel_get_dropping, NULL, NULL, NULL},
    {NULL, NULL, NULL, NULL, NULL},
};

PyTypeObject CoDelType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.ControlledDelay",
    sizeof(CoDelOb),
};

static void
codel_type_init(void)
{
    CoDelType.tp_dealloc = CoDel_dealloc;
    CoDelType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    CoDelType.tp_traverse = CoDel_traverse;
    CoDelType.tp_clear = CoDel_clear_;
    CoDelType.tp_methods = CoDel_methods;
    CoDelType.tp_members = CoDel_members;
    CoDelType.tp_getset = CoDel_getset;
    CoDelType.tp_new = CoDel_new;
}

/* ------------------------------------------------------------------ */
/* SlotDispatch: the pool's per-slot stateChanged listener             */
/* (pool._slot_state_changed) with the idle-feed and busy no-op fast   */
/* paths in C; every other state (and every unusual condition)         */
/* delegates to the Python method, which remains the full logic.       */

PyObject *s_p_backends;          /* "p_backends" */
PyObject *s_p_dead;              /* "p_dead" */
PyObject *s_connected_to_backend;/* "connectedToBackend" */
PyObject *s_slot_state_changed;  /* "_slot_state_changed" */
PyObject *s_remove_node;         /* "remove" */
PyObject *s_rebalance;           /* "rebalance" */
PyObject *s_set_unwanted;        /* "set_unwanted" */

typedef struct {
    PyObject_HEAD
    PyObject *sd_pool;      /* owned */
    PyObject *sd_fsm;       /* the slot (FSMOb), owned */
    PyObject *sd_key;       /* owned */
    NQueue *sd_idleq;       /* owned (never replaced by the pool) */
    NQueue *sd_waiters;     /* owned */
    PyObject *sd_codel;     /* owned native ControlledDelay or NULL */
    int sd_has_codel;       /* codel configured but not native =>
                             * python path */
    vectorcallfunc sd_vectorcall;
} SlotDispatch;

extern PyTypeObject SlotDispatchType;

static int
sd_fallback(SlotDispatch *d, PyObject *st)
{
    PyObject *r = PyObject_CallMethodObjArgs(
        d->sd_pool, s_slot_state_changed, d->sd_fsm, d->sd_key, st,
        NULL);
    if (r == NULL)
        return -1;
    Py_DECREF(r);
    return 0;
}

static PyObject *
slotdispatch_run(PyObject *self_, PyObject *st)
{
    SlotDispatch *d = (SlotDispatch *)self_;
    FSMOb *fsm = (FSMOb *)d->sd_fsm;

    /* common preconditions for both fast paths */
    SlotOb *so = (SlotOb *)d->sd_fsm;
    int in_initq = slot_field_set(&so->sl_initq_node);

    if (!in_initq &&
        (st == s_busy_st ||
         (PyUnicode_Check(st) &&
          PyUnicode_Compare(st, s_busy_st) == 0))) {
        /* busy: with no pinger handle and no stale idleq node this
         * dispatch is a no-op */
        if (!slot_field_set(&so->sl_idleq_node)) {
            PyObject *hdl = so->sl_handle;
            int pinger = 0;
            if (hdl != NULL && hdl != Py_None &&
                is_handle(hdl))
                pinger = ((CHOb *)hdl)->chb_pinger;
            if (!pinger)
                Py_RETURN_NONE;
        }
        if (sd_fallback(d, st) < 0)
            return NULL;
        Py_RETURN_NONE;
    }

    if (!in_initq && (!d->sd_has_codel || d->sd_codel != NULL) &&
        (st == s_idle ||
         (PyUnicode_Check(st) &&
          PyUnicode_Compare(st, s_idle) == 0))) {
        PoolCtx *cx = pool_ctx(d->sd_pool);
        PyObject *dead;
        if (cx != NULL) {
            dead = cx->pc_dead;
            Py_INCREF(dead);
        } else {
            dead = PyObject_GetAttr(d->sd_pool, s_p_dead);
        }
        if (dead == NULL)
            return NULL;
        int isdead = PyDict_Check(dead) ?
            PyDict_Contains(dead, d->sd_key) : 1;
        Py_DECREF(dead);
        if (isdead != 0) {
            /* dead-backend recovery (or error): python path */
            if (isdead < 0)
                return NULL;
            if (sd_fallback(d, st) < 0)
                return NULL;
            Py_RETURN_NONE;
        }
        /* emit connectedToBackend (cheap when nobody listens) */
        PyObject *eargs[3] = {s_connected_to_backend, d->sd_key,
                              d->sd_fsm};
        if (emitter_emit_core((Emitter *)d->sd_pool, eargs[0],
                              eargs + 1, 2) < 0)
            return NULL;
        /* still idle? (stale events tolerated) */
        PyObject *fs = fsm->f_state;
        if (!(fs == s_idle ||
              (fs != NULL && PyUnicode_Compare(fs, s_idle) == 0))) {
            /* the event already emitted above; only the trailing
             * was-idle-now-isn't unlink branch can still apply */
            if (slot_field_set(&so->sl_idleq_node)) {
                PyObject *idn = so->sl_idleq_node;
                Py_INCREF(idn);
                PyObject *rr = PyObject_CallMethodObjArgs(
                    idn, s_remove_node, NULL);
                Py_DECREF(idn);
                if (rr == NULL)
                    return NULL;
                Py_DECREF(rr);
                slot_field_store(&so->sl_idleq_node, Py_None);
                PyObject *rb = PyObject_CallMethodObjArgs(
                    d->sd_pool, s_rebalance, NULL);
                if (rb == NULL)
                    return NULL;
                Py_DECREF(rb);
            }
            Py_RETURN_NONE;
        }
        {
            PyObject *backends = PyObject_GetAttr(d->sd_pool,
                                                  s_p_backends);
            if (backends == NULL)
                return NULL;
            int wanted = PyDict_Check(backends) ?
                PyDict_Contains(backends, d->sd_key) : 0;
            Py_DECREF(backends);
            if (wanted < 0)
                return NULL;
            if (!wanted) {
                /* no longer a backend: set_unwanted, like the python
                 * dispatcher (it has not emitted again: call the slot
                 * method directly) */
                PyObject *su = PyObject_CallMethodObjArgs(
                    d->sd_fsm, s_set_unwanted, NULL);
                if (su == NULL)
                    return NULL;
                Py_DECREF(su);
                Py_RETURN_NONE;
            }
        }
        /* feed waiters (with the CoDel drop check on each; like the
         * python dispatcher, overloaded() is fed BEFORE the staleness
         * check so the controller sees every dequeue) */
        while (d->sd_waiters->q_len > 0) {
            PyObject *hdl = nqueue_shift_value(d->sd_waiters);
            if (hdl == NULL)
                return NULL;
            if (!is_handle(hdl)) {
                Py_DECREF(hdl);
                continue;
            }
            int drop = 0;
            if (d->sd_codel != NULL) {
                drop = codel_overloaded_c((CoDelOb *)d->sd_codel,
                                          ((CHOb *)hdl)->chb_started);
                if (drop < 0) {
                    Py_DECREF(hdl);
                    return NULL;
                }
            }
            if (!ch_state_is((CHOb *)hdl, s_waiting)) {
                Py_DECREF(hdl);
                continue;
            }
            if (drop) {
                PyObject *r = CH_timeout(hdl, NULL);
                Py_DECREF(hdl);
                if (r == NULL)
                    return NULL;
                Py_DECREF(r);
                continue;
            }
            PyObject *r = CH_try_(hdl, d->sd_fsm);
            Py_DECREF(hdl);
            if (r == NULL)
                return NULL;
            Py_DECREF(r);
            Py_RETURN_NONE;
        }
        if (d->sd_codel != NULL &&
            codel_empty_c((CoDelOb *)d->sd_codel) < 0)
            return NULL;
        /* no waiter: park on the idle queue */
        QNode *n = nqueue_push(d->sd_idleq, d->sd_fsm);
        if (n == NULL)
            return NULL;
        Py_XSETREF(so->sl_idleq_node, (PyObject *)n);
        Py_RETURN_NONE;
    }

    if (sd_fallback(d, st) < 0)
        return NULL;
    Py_RETURN_NONE;
}

static PyObject *
SlotDispatch_call(PyObject *self_, PyObject *args, PyObject *kwds)
{
    (void)kwds;
    if (PyTuple_GET_SIZE(args) != 1) {
        PyErr_SetString(PyExc_TypeError, "SlotDispatch(state)");
        return NULL;
    }
    return slotdispatch_run(self_, PyTuple_GET_ITEM(args, 0));
}

static PyObject *
SlotDispatch_vectorcall(PyObject *self_, PyObject *const *args,
                        size_t nargsf, PyObject *kwnames)
{
    if (PyVectorcall_NARGS(nargsf) != 1 ||
        (kwnames != NULL && PyTuple_GET_SIZE(kwnames) != 0)) {
        PyErr_SetString(PyExc_TypeError, "SlotDispatch(state)");
        return NULL;
    }
    return slotdispatch_run(self_, args[0]);
}

static int
SlotDispatch_traverse(PyObject *self_, visitproc visit, void *arg)
{
    SlotDispatch *d = (SlotDispatch *)self_;
    Py_VISIT(d->sd_pool);
    Py_VISIT(d->sd_fsm);
    Py_VISIT(d->sd_key);
    Py_VISIT((PyObject *)d->sd_idleq);
    Py_VISIT((PyObject *)d->sd_waiters);
    Py_VISIT(d->sd_codel);
    return 0;
}

static int
SlotDispatch_clear_(PyObject *self_)
{
    SlotDispatch *d = (SlotDispatch *)self_;
    Py_CLEAR(d->sd_pool);
    Py_CLEAR(d->sd_fsm);
    Py_CLEAR(d->sd_key);
    Py_CLEAR(d->sd_idleq);
    Py_CLEAR(d->sd_waiters);
    Py_CLEAR(d->sd_codel);
    return 0;
}

static void
SlotDispatch_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    SlotDispatch_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyObject *
SlotDispatch_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    PyObject *pool, *fsm, *key, *has_codel;
    (void)kwds;
    if (!PyArg_ParseTuple(args, "OOOO", &pool, &fsm, &key, &has_codel))
        return NULL;
    if (!PyObject_TypeCheck(pool, &EmitterType) ||
        !is_slot(fsm)) {
        PyErr_SetString(PyExc_TypeError,
                        "SlotDispatch(pool, slot, key, has_codel)");
        return NULL;
    }
    PyObject *iq = PyObject_GetAttrString(pool, "p_idleq");
    PyObject *wq = iq ? PyObject_GetAttrString(pool, "p_waiters") : NULL;
    if (wq == NULL || !PyObject_TypeCheck(iq, &NQueueType) ||
        !PyObject_TypeCheck(wq, &NQueueType)) {
        Py_XDECREF(iq);
        Py_XDECREF(wq);
        if (!PyErr_Occurred())
            PyErr_SetString(PyExc_TypeError,
                            "pool queues must be native");
        return NULL;
    }
    SlotDispatch *d = PyObject_GC_New(SlotDispatch, type);
    if (d == NULL) {
        Py_DECREF(iq);
        Py_DECREF(wq);
        return NULL;
    }
    Py_INCREF(pool);
    d->sd_pool = pool;
    Py_INCREF(fsm);
    d->sd_fsm = fsm;
    Py_INCREF(key);
    d->sd_key = key;
    d->sd_idleq = (NQueue *)iq;
    d->sd_waiters = (NQueue *)wq;
    d->sd_has_codel = PyObject_IsTrue(has_codel);
    d->sd_codel = NULL;
    d->sd_vectorcall = SlotDispatch_vectorcall;
    PyObject_GC_Track((PyObject *)d);
    if (d->sd_has_codel) {
        PyObject *cd = PyObject_GetAttrString(pool, "p_codel");
        if (cd == NULL) {
            PyErr_Clear();
        } else if (PyObject_TypeCheck(cd, &CoDelType)) {
            d->sd_codel = cd;     /* native: feed path stays in C */
        } else {
            Py_DECREF(cd);        /* pure codel: python feed path */
        }
    }
    return (PyObject *)d;
}

PyTypeObject SlotDispatchType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.SlotDispatch",
    sizeof(SlotDispatch),
};

/* -- SlotKit type ---------------------------------------------------- */

static int
SlotKit_traverse(PyObject *self_, visitproc visit, void *arg)
{
    SlotKit *k = (SlotKit *)self_;
    Py_VISIT((PyObject *)k->k_slot);
    Py_VISIT(k->k_smgr);
    Py_VISIT(k->k_observed);
    for (int i = 0; i < KCB_N; i++)
        Py_VISIT(k->k_cbs[i]);
    return 0;
}

static int
SlotKit_clear_(PyObject *self_)
{
    SlotKit *k = (SlotKit *)self_;
    Py_CLEAR(k->k_slot);
    Py_CLEAR(k->k_smgr);
    Py_CLEAR(k->k_observed);
    for (int i = 0; i < KCB_N; i++)
        Py_CLEAR(k->k_cbs[i]);
    return 0;
}

static void
SlotKit_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    SlotKit_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyObject *
SlotKit_new(PyTypeObject *type, PyObject *args, PyObject *kwds)
{
    PyObject *slot, *smgr;
    (void)kwds;
    if (!PyArg_ParseTuple(args, "OO", &slot, &smgr))
        return NULL;
    if (!is_slot(slot) ||
        !is_fsm(smgr)) {
        PyErr_SetString(PyExc_TypeError,
                        "SlotKit(slot, smgr): a SlotBase and a native "
                        "FSM required");
        return NULL;
    }
    SlotKit *k = PyObject_GC_New(SlotKit, type);
    if (k == NULL)
        return NULL;
    Py_INCREF(slot);
    k->k_slot = (FSMOb *)slot;
    Py_INCREF(smgr);
    k->k_smgr = smgr;
    k->k_observed = NULL;
    k->k_busy_serial = 0;
    k->k_idle_serial = 0;
    for (int i = 0; i < KCB_N; i++)
        k->k_cbs[i] = NULL;
    PyObject_GC_Track((PyObject *)k);
    for (int i = 0; i < KCB_N; i++) {
        KitCb *cb = PyObject_GC_New(KitCb, &KitCbType);
        if (cb == NULL) {
            Py_DECREF((PyObject *)k);
            return NULL;
        }
        Py_INCREF((PyObject *)k);
        cb->kc_kit = k;
        cb->kc_which = i;
        cb->kc_vectorcall = KitCb_vectorcall;
        PyObject_GC_Track((PyObject *)cb);
        k->k_cbs[i] = (PyObject *)cb;
    }
#if CUEBALL_SLOT_HOOKS
    /* the socket manager's emissions call this kit (slotkit_smgr_hook) */
    Py_INCREF((PyObject *)k);
    Py_XSETREF(((FSMOb *)smgr)->f_watchkit, (PyObject *)k);
#endif
    return (PyObject *)k;
}

PyTypeObject SlotKitType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed.SlotKit",
    sizeof(SlotKit),
};

static void
slotkit_types_init(void)
{
    KitCbType.tp_dealloc = KitCb_dealloc;
    KitCbType.tp_call = KitCb_call;
    KitCbType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    KitCbType.tp_traverse = KitCb_traverse;
    KitCbType.tp_clear = KitCb_clear_;
    /* all of the kit's callbacks are the library's own: they answer
     * _cueball_internal like _ConnErrCb, whose job one of them does */
    KitCbType.tp_getset = ConnErrCb_getset;

    SlotKitType.tp_dealloc = SlotKit_dealloc;
    SlotKitType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    SlotKitType.tp_traverse = SlotKit_traverse;
    SlotKitType.tp_clear = SlotKit_clear_;
    SlotKitType.tp_new = SlotKit_new;

    SlotDispatchType.tp_dealloc = SlotDispatch_dealloc;
    SlotDispatchType.tp_call = SlotDispatch_call;
    SlotDispatchType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC;
    SlotDispatchType.tp_traverse = SlotDispatch_traverse;
    SlotDispatchType.tp_clear = SlotDispatch_clear_;
    SlotDispatchType.tp_new = SlotDispatch_new;

    SlotBaseType.tp_methods = Slot_methods;
#if CUEBALL_VECTORCALL
    /* emission and the event loop call these without building a tuple */
    KitCbType.tp_vectorcall_offset = offsetof(KitCb, kc_vectorcall);
    KitCbType.tp_flags |= Py_TPFLAGS_HAVE_VECTORCALL;
    SlotDispatchType.tp_vectorcall_offset =
        offsetof(SlotDispatch, sd_vectorcall);
    SlotDispatchType.tp_flags |= Py_TPFLAGS_HAVE_VECTORCALL;
    FlushBatchType.tp_vectorcall_offset = offsetof(FlushBatch, fb_vectorcall);
    FlushBatchType.tp_flags |= Py_TPFLAGS_HAVE_VECTORCALL;
#endif
}

/* ------------------------------------------------------------------ */
/* ClaimMethod: ConnectionPool.claim as a method descriptor.  The      */
/* positional claim({}, cb) / claim(None, cb) on a running pool        */
/* without CoDel goes straight to pool_claim, with no Python frame;    */
/* every other shape (keywords, options, claim(cb), CoDel, a pool that */
/* is not running) calls the Python function it wraps, unchanged.      */

PyObject *s_p_codel;             /* "p_codel" */
PyObject *s_p_claim_log;         /* "p_claim_log" */

typedef struct {
    PyObject_HEAD
    PyObject *cm_func;           /* the Python ConnectionPool.claim */
    PyObject *cm_handle_cls;     /* ClaimHandle */
    PyObject *cm_doc;
    PyObject *cm_name;
    PyObject *cm_qualname;
    PyObject *cm_module;
    vectorcallfunc cm_vectorcall;
} ClaimMethod;

extern PyTypeObject ClaimMethodType;

static PyObject *
ClaimMethod_vectorcall(PyObject *self_, PyObject *const *args,
                       size_t nargsf, PyObject *kwnames)
{
    ClaimMethod *cm = (ClaimMethod *)self_;
    if (PyVectorcall_NARGS(nargsf) == 3 &&
        (kwnames == NULL || PyTuple_GET_SIZE(kwnames) == 0)) {
        PyObject *pool = args[0], *opt = args[1], *cb = args[2];
        if (cb != Py_None &&
            (opt == Py_None ||
             (PyDict_CheckExact(opt) && PyDict_GET_SIZE(opt) == 0)) &&
            is_fsm(pool)) {
            PyObject *pst = ((FSMOb *)pool)->f_state;
            int open = pst != NULL &&
                (pst == s_running_st ||
                 PyUnicode_Compare(pst, s_running_st) == 0 ||
                 PyUnicode_CompareWithASCIIString(pst, "starting") == 0);
            PoolCtx *cx = open ? pool_ctx(pool) : NULL;
            if (cx != NULL) {
                if (cx->pc_no_codel) {
                    PyObject *pargs[5] = {cm->cm_handle_cls, pool, cb,
                                          cx->pc_log,
                                          ((FSMOb *)pool)->f_loop};
                    return speed_pool_claim(NULL, pargs, 5);
                }
                return PyObject_Vectorcall(cm->cm_func, args, nargsf,
                                           kwnames);
            }
            /* no context (not a ConnectionPool): the attributes */
            PyObject *codel = open ? PyObject_GetAttr(pool, s_p_codel)
                                   : NULL;
            if (open && codel == NULL)
                return NULL;
            Py_XDECREF(codel);
            if (open && codel == Py_None) {
                PyObject *log = PyObject_GetAttr(pool, s_p_claim_log);
                if (log == NULL)
                    return NULL;
                PyObject *pargs[5] = {cm->cm_handle_cls, pool, cb, log,
                                      ((FSMOb *)pool)->f_loop};
                PyObject *h = speed_pool_claim(NULL, pargs, 5);
                Py_DECREF(log);
                return h;
            }
        }
    }
    return PyObject_Vectorcall(cm->cm_func, args, nargsf, kwnames);
}

static PyObject *
ClaimMethod_descr_get(PyObject *self_, PyObject *obj, PyObject *type)
{
    (void)type;
    if (obj == NULL || obj == Py_None) {
        Py_INCREF(self_);
        return self_;
    }
    return PyMethod_New(self_, obj);
}

static int
ClaimMethod_traverse(PyObject *self_, visitproc visit, void *arg)
{
    ClaimMethod *cm = (ClaimMethod *)self_;
    Py_VISIT(cm->cm_func);
    Py_VISIT(cm->cm_handle_cls);
    return 0;
}

static int
ClaimMethod_clear_(PyObject *self_)
{
    ClaimMethod *cm = (ClaimMethod *)self_;
    Py_CLEAR(cm->cm_func);
    Py_CLEAR(cm->cm_handle_cls);
    Py_CLEAR(cm->cm_doc);
    Py_CLEAR(cm->cm_name);
    Py_CLEAR(cm->cm_qualname);
    Py_CLEAR(cm->cm_module);
    return 0;
}

static void
ClaimMethod_dealloc(PyObject *self_)
{
    PyObject_GC_UnTrack(self_);
    ClaimMethod_clear_(self_);
    PyObject_GC_Del(self_);
}

static PyMemberDef ClaimMethod_members[] = {
    {(char *)"__wrapped__", T_OBJECT, offsetof(ClaimMethod, cm_func),
     READONLY, NULL},
    {(char *)"__doc__", T_OBJECT, offsetof(ClaimMethod, cm_doc), READONLY,
     NULL},
    {(char *)"__name__", T_OBJECT, offsetof(ClaimMethod, cm_name), READONLY,
     NULL},
    {(char *)"__qualname__", T_OBJECT, offsetof(ClaimMethod, cm_qualname),
     READONLY, NULL},
    {(char *)"__module__", T_OBJECT, offsetof(ClaimMethod, cm_module),
     READONLY, NULL},
    {NULL, 0, 0, 0, NULL},
};

PyTypeObject ClaimMethodType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    "cueball_amd._speed._ClaimMethod",
    sizeof(ClaimMethod),
};

static void
claim_method_type_init(void)
{
    ClaimMethodType.tp_dealloc = ClaimMethod_dealloc;
    ClaimMethodType.tp_vectorcall_offset =
        offsetof(ClaimMethod, cm_vectorcall);
    ClaimMethodType.tp_call = PyVectorcall_Call;
    ClaimMethodType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC |
        Py_TPFLAGS_HAVE_VECTORCALL | Py_TPFLAGS_METHOD_DESCRIPTOR;
    ClaimMethodType.tp_traverse = ClaimMethod_traverse;
    ClaimMethodType.tp_clear = ClaimMethod_clear_;
    ClaimMethodType.tp_members = ClaimMethod_members;
    ClaimMethodType.tp_descr_get = ClaimMethod_descr_get;
}

/* claim_method(func, handle_cls) -> the descriptor to put on the pool
 * class in place of func (func itself in a build without the entry) */
static PyObject *
speed_claim_method(PyObject *mod, PyObject *const *args, Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 2 || !PyCallable_Check(args[0]) || !PyType_Check(args[1]) ||
        !PyType_IsSubtype((PyTypeObject *)args[1], &CHType)) {
        PyErr_SetString(PyExc_TypeError,
                        "claim_method(func, ClaimHandleBase subclass)");
        return NULL;
    }
#if !CUEBALL_VECTORCALL
    Py_INCREF(args[0]);
    return args[0];
#else
    ClaimMethod *cm = PyObject_GC_New(ClaimMethod, &ClaimMethodType);
    if (cm == NULL)
        return NULL;
    Py_INCREF(args[0]);
    cm->cm_func = args[0];
    Py_INCREF(args[1]);
    cm->cm_handle_cls = args[1];
    cm->cm_vectorcall = ClaimMethod_vectorcall;
    cm->cm_doc = PyObject_GetAttrString(args[0], "__doc__");
    cm->cm_name = PyObject_GetAttrString(args[0], "__name__");
    cm->cm_qualname = PyObject_GetAttrString(args[0], "__qualname__");
    cm->cm_module = PyObject_GetAttrString(args[0], "__module__");
    PyErr_Clear();               /* a callable without one: reads None */
    PyObject_GC_Track((PyObject *)cm);
    return (PyObject *)cm;
#endif
}

/* _set_cycle_classes(handle_cls, slot_cls, pool_cls): the Python classes
 * whose instances walk the claim cycle, for the exact-type tests
 * (is_handle, is_slot, is_fsm).  None leaves a class as it is. */
static PyObject *
speed_set_cycle_classes(PyObject *mod, PyObject *const *args,
                        Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 3) {
        PyErr_SetString(PyExc_TypeError,
                        "_set_cycle_classes(handle_cls, slot_cls, pool_cls)");
        return NULL;
    }
    PyTypeObject *bases[3] = {&CHType, &SlotBaseType, &FSMType};
    PyTypeObject **dst[3] = {&g_handle_cls, &g_slot_cls, &g_pool_cls};
    for (int i = 0; i < 3; i++) {
        if (args[i] == Py_None)
            continue;
        PyTypeObject *cls = (PyTypeObject *)args[i];
        if (!PyType_Check(args[i]) || !PyType_IsSubtype(cls, bases[i]) ||
            (i > 0 && PyType_IsSubtype(cls, &CHType)) ||
            (i == 2 && PyType_IsSubtype(cls, &SlotBaseType))) {
            PyErr_SetString(PyExc_TypeError,
                "_set_cycle_classes: a ClaimHandleBase, a SlotBase and a "
                "plain FSM subclass required");
            return NULL;
        }
    }
    for (int i = 0; i < 3; i++) {
        if (args[i] == Py_None)
            continue;
        Py_INCREF(args[i]);
        PyTypeObject *old = *dst[i];
        *dst[i] = (PyTypeObject *)args[i];
        Py_XDECREF((PyObject *)old);
    }
    Py_RETURN_NONE;
}

/* _debug_cycle_state(emitter=None): what the per-claim caches hold, for
 * the tests.  With an emitter, "leak_cache" is None or the cached counts
 * of its leak detector if they are valid. */
static PyObject *
speed_debug_cycle_state(PyObject *mod, PyObject *const *args,
                        Py_ssize_t nargs)
{
    (void)mod;
    PyObject *lk = Py_None;
    Py_INCREF(lk);
    if (nargs >= 1 && PyObject_TypeCheck(args[0], &EmitterType)) {
        LeakCache *c = ((Emitter *)args[0])->ev_lk;
        if (c != NULL && c->lk_ok &&
            c->lk_gen == ((Emitter *)args[0])->ev_gen) {
            Py_DECREF(lk);
            lk = Py_BuildValue("(llll)", c->lk_cnt[0], c->lk_cnt[1],
                               c->lk_cnt[2], c->lk_cnt[3]);
            if (lk == NULL)
                return NULL;
        }
    }
    return Py_BuildValue("{s:N,s:i,s:i}",
                         "leak_cache", lk,
                         "leak_tag", (int)CUEBALL_LEAK_TAG,
                         "own_conn_err", (int)CUEBALL_OWN_CONN_ERR);
}

PyObject *
speed_set_tracer(PyObject *mod, PyObject *fn)
{
    (void)mod;
    if (fn == Py_None) {
        Py_CLEAR(g_tracer);
    } else {
        Py_INCREF(fn);
        Py_XSETREF(g_tracer, fn);
    }
    Py_RETURN_NONE;
}

/* ------------------------------------------------------------------ */
/* Key affinity (cueball_amd/affinity.py holds the definition and the  */
/* Python twins): what a keyed claim computes on every try.            */

static inline uint64_t
aff_fnv1a64(const unsigned char *p, Py_ssize_t n)
{
    uint64_t h = 0xcbf29ce484222325ULL;
    for (Py_ssize_t i = 0; i < n; i++)
        h = (h ^ p[i]) * 0x100000001b3ULL;
    return h;
}

static inline uint64_t
aff_mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return z;
}

/* affinity_hash(bytes) -> int: FNV-1a, 64 bits */
static PyObject *
speed_affinity_hash(PyObject *mod, PyObject *data)
{
    (void)mod;
    if (!PyBytes_Check(data)) {
        PyErr_SetString(PyExc_TypeError, "affinity_hash: bytes required");
        return NULL;
    }
    return PyLong_FromUnsignedLongLong(aff_fnv1a64(
        (const unsigned char *)PyBytes_AS_STRING(data),
        PyBytes_GET_SIZE(data)));
}

/* affinity_rank(bytes, tuple of backend hashes) -> tuple of indices by
 * descending score, best first; equal scores keep their input order */
static PyObject *
speed_affinity_rank(PyObject *mod, PyObject *const *args, Py_ssize_t nargs)
{
    (void)mod;
    if (nargs != 2 || !PyBytes_Check(args[0]) || !PyTuple_Check(args[1])) {
        PyErr_SetString(PyExc_TypeError,
            "affinity_rank: bytes and a tuple of backend hashes required");
        return NULL;
    }
    uint64_t kh = aff_fnv1a64(
        (const unsigned char *)PyBytes_AS_STRING(args[0]),
        PyBytes_GET_SIZE(args[0]));
    Py_ssize_t n = PyTuple_GET_SIZE(args[1]);
    uint64_t sbuf[32];
    Py_ssize_t ibuf[32];
    uint64_t *sc = sbuf;
    Py_ssize_t *ix = ibuf;
    if (n > 32) {
        sc = (uint64_t *)PyMem_Malloc((size_t)n * sizeof(uint64_t));
        ix = (Py_ssize_t *)PyMem_Malloc((size_t)n * sizeof(Py_ssize_t));
        if (sc == NULL || ix == NULL) {
            PyMem_Free(sc);
            PyMem_Free(ix);
            return PyErr_NoMemory();
        }
    }
    PyObject *out = NULL;
    Py_ssize_t i;
    for (i = 0; i < n; i++) {
        uint64_t h = PyLong_AsUnsignedLongLong(PyTuple_GET_ITEM(args[1], i));
        if (h == (uint64_t)-1 && PyErr_Occurred())
            goto done;
        /* a stable insertion sort: the backends of a pool are few */
        uint64_t s = aff_mix64(kh ^ h);
        Py_ssize_t j = i;
        while (j > 0 && sc[j - 1] < s) {
            sc[j] = sc[j - 1];
            ix[j] = ix[j - 1];
            j--;
        }
        sc[j] = s;
        ix[j] = i;
    }
    out = PyTuple_New(n);
    if (out == NULL)
        goto done;
    for (i = 0; i < n; i++) {
        PyObject *v = PyLong_FromSsize_t(ix[i]);
        if (v == NULL) {
            Py_CLEAR(out);
            goto done;
        }
        PyTuple_SET_ITEM(out, i, v);
    }
done:
    if (sc != sbuf) {
        PyMem_Free(sc);
        PyMem_Free(ix);
    }
    return out;
}

PyMethodDef speed_methods[] = {
    {"affinity_hash", speed_affinity_hash, METH_O, NULL},
    {"affinity_rank", (PyCFunction)(void (*)(void))speed_affinity_rank,
     METH_FASTCALL, NULL},
    {"_set_claim_helpers",
     (PyCFunction)(void (*)(void))speed_set_claim_helpers, METH_FASTCALL,
     NULL},
    {"_set_tracer", speed_set_tracer, METH_O, NULL},
    {"_set_stack_traces",
     (PyCFunction)(void (*)(void))speed_set_stack_traces, METH_FASTCALL,
     NULL},
    {"count_listeners",
     (PyCFunction)(void (*)(void))speed_count_listeners, METH_FASTCALL,
     NULL},
    {"_set_helpers", (PyCFunction)(void (*)(void))speed_set_helpers,
     METH_FASTCALL, NULL},
    {"claim_fast", (PyCFunction)(void (*)(void))speed_claim_fast,
     METH_FASTCALL, NULL},
    {"pool_claim", (PyCFunction)(void (*)(void))speed_pool_claim,
     METH_FASTCALL, NULL},
    {"claim_method", (PyCFunction)(void (*)(void))speed_claim_method,
     METH_FASTCALL, NULL},
    {"_set_cycle_classes",
     (PyCFunction)(void (*)(void))speed_set_cycle_classes, METH_FASTCALL,
     NULL},
    {"_debug_cycle_state",
     (PyCFunction)(void (*)(void))speed_debug_cycle_state, METH_FASTCALL,
     NULL},
    {NULL, NULL, 0, NULL},
};

struct PyModuleDef speedmodule = {
    PyModuleDef_HEAD_INIT,
    "cueball_amd._speed",
    "Native event/FSM runtime core",
    -1,
    speed_methods,
};

}  /* namespace */

PyMODINIT_FUNC
PyInit__speed(void)
{
    s_stateChanged = PyUnicode_InternFromString("stateChanged");
    s_listener = PyUnicode_InternFromString("listener");
    s_on = PyUnicode_InternFromString("on");
    s_remove_listener = PyUnicode_InternFromString("remove_listener");
    s_call_soon = PyUnicode_InternFromString("call_soon");
    s_call_later = PyUnicode_InternFromString("call_later");
    s_cancel = PyUnicode_InternFromString("cancel");
    s_state_prefix = PyUnicode_InternFromString("state_");
    s_dot = PyUnicode_InternFromString(".");
    s_underscore = PyUnicode_InternFromString("_");
    s_flush_name = PyUnicode_InternFromString("_flush_state_changed");
    s_internal = PyUnicode_InternFromString("_cueball_internal");
    s_is_closed = PyUnicode_InternFromString("is_closed");
    s_claim = PyUnicode_InternFromString("claim");
    s_warn = PyUnicode_InternFromString("warn");
    s_incr = PyUnicode_InternFromString("_incr_counter");
    s_claim_timeout_evt = PyUnicode_InternFromString("claim-timeout");
    s_is_in_state = PyUnicode_InternFromString("is_in_state");
    s_time = PyUnicode_InternFromString("time");
    s_waiting = PyUnicode_InternFromString("waiting");
    s_claiming = PyUnicode_InternFromString("claiming");
    s_claimed = PyUnicode_InternFromString("claimed");
    s_released = PyUnicode_InternFromString("released");
    s_closed = PyUnicode_InternFromString("closed");
    s_cancelled = PyUnicode_InternFromString("cancelled");
    s_failed = PyUnicode_InternFromString("failed");
    s_idle = PyUnicode_InternFromString("idle");
    s_error_evt = PyUnicode_InternFromString("error");
    t_waiting_valid = PyTuple_Pack(3, s_claiming, s_cancelled, s_failed);
    t_claiming_valid = PyTuple_Pack(3, s_claimed, s_waiting, s_cancelled);
    t_claimed_valid = PyTuple_Pack(2, s_released, s_closed);
    t_empty = PyTuple_New(0);
    s_leak_events[0] = PyUnicode_InternFromString("close");
    s_leak_events[1] = s_error_evt;
    s_leak_events[2] = PyUnicode_InternFromString("readable");
    s_leak_events[3] = PyUnicode_InternFromString("data");
    g_entry_name_cache = PyDict_New();
    if (g_entry_name_cache == NULL)
        return NULL;
    g_flush_batches = PyDict_New();
    if (g_flush_batches == NULL)
        return NULL;

    s_running_st = PyUnicode_InternFromString("running");
    s_p_idleq_node = PyUnicode_InternFromString("p_idleq_node");
    s_p_total_conns = PyUnicode_InternFromString("p_total_conns");
    s_p_busy_hwm = PyUnicode_InternFromString("p_busy_hwm");
    s_p_demand_hwm = PyUnicode_InternFromString("p_demand_hwm");
    s_ticket_slow = PyUnicode_InternFromString("_ticket_slow");
    s_p_idleq = PyUnicode_InternFromString("p_idleq");
    s_p_waiters = PyUnicode_InternFromString("p_waiters");
    s_p_initq = PyUnicode_InternFromString("p_initq");
    s_p_counters = PyUnicode_InternFromString("p_counters");
    s_p_rebal_scheduled = PyUnicode_InternFromString("p_rebal_scheduled");
    s_max_claim_queue = PyUnicode_InternFromString("max-claim-queue");
    s_queued_claim = PyUnicode_InternFromString("queued-claim");
    s_connected_st = PyUnicode_InternFromString("connected");
    s_busy_st = PyUnicode_InternFromString("busy");
    s_stopping_st = PyUnicode_InternFromString("stopping");
    s_stopped_st = PyUnicode_InternFromString("stopped");
    s_retrying_st = PyUnicode_InternFromString("retrying");
    s_connecting_st = PyUnicode_InternFromString("connecting");
    s_killing_st = PyUnicode_InternFromString("killing");
    s_unwanted_evt = PyUnicode_InternFromString("unwanted");
    s_sm_socket = PyUnicode_InternFromString("sm_socket");
    t_busy_valid = PyTuple_Pack(6, s_idle, s_stopping_st, s_stopped_st,
                                s_retrying_st, s_killing_st,
                                s_connecting_st);
    t_idle_valid = PyTuple_Pack(5, s_retrying_st, s_connecting_st,
                                s_stopping_st, s_stopped_st, s_busy_st);
    s_p_backends = PyUnicode_InternFromString("p_backends");
    s_p_dead = PyUnicode_InternFromString("p_dead");
    s_connected_to_backend =
        PyUnicode_InternFromString("connectedToBackend");
    s_slot_state_changed =
        PyUnicode_InternFromString("_slot_state_changed");
    s_remove_node = PyUnicode_InternFromString("remove");
    s_rebalance = PyUnicode_InternFromString("rebalance");
    s_set_unwanted = PyUnicode_InternFromString("set_unwanted");
    queue_types_init();
    poolctx_type_init();
    ct_type_init();
    slotkit_types_init();
    codel_type_init();
    claim_method_type_init();
    s_p_codel = PyUnicode_InternFromString("p_codel");
    s_p_claim_log = PyUnicode_InternFromString("p_claim_log");
    s_p_lat = PyUnicode_InternFromString("p_lat");
    latency_types_init();
    if (PyType_Ready(&LatHistType) < 0 ||
        PyType_Ready(&PoolLatType) < 0)
        return NULL;
    if (PyType_Ready(&EmitterType) < 0 ||
        PyType_Ready(&OnceWrapperType) < 0 ||
        PyType_Ready(&GuardedCbType) < 0 ||
        PyType_Ready(&ScopeType) < 0 ||
        PyType_Ready(&IntervalType) < 0 ||
        PyType_Ready(&FlushBatchType) < 0 ||
        PyType_Ready(&ConnErrCbType) < 0 ||
        PyType_Ready(&FailCbType) < 0 ||
        PyType_Ready(&CHType) < 0 ||
        PyType_Ready(&FSMType) < 0 ||
        PyType_Ready(&SlotBaseType) < 0 ||
        PyType_Ready(&QNodeType) < 0 ||
        PyType_Ready(&NQueueType) < 0 ||
        PyType_Ready(&PoolCtxType) < 0 ||
        PyType_Ready(&CTType) < 0 ||
        PyType_Ready(&KitCbType) < 0 ||
        PyType_Ready(&SlotKitType) < 0 ||
        PyType_Ready(&SlotDispatchType) < 0 ||
        PyType_Ready(&ClaimMethodType) < 0 ||
        PyType_Ready(&CoDelType) < 0)
        return NULL;

    g_remove_desc = PyDict_GetItemString(EmitterType.tp_dict,
                                         "remove_listener");
    if (g_remove_desc == NULL)
        return NULL;
    Py_INCREF(g_remove_desc);
    g_ch_remove_desc = PyDict_GetItemString(CHType.tp_dict,
                                            "remove_listener");
    if (g_ch_remove_desc == NULL)
        return NULL;
    Py_INCREF(g_ch_remove_desc);
    if (ch_entries_init() < 0)
        return NULL;
    g_inf = PyFloat_FromDouble(HUGE_VAL);
    if (g_inf == NULL)
        return NULL;

    PyObject *m = PyModule_Create(&speedmodule);
    if (m == NULL)
        return NULL;
    Py_INCREF(&EmitterType);
    PyModule_AddObject(m, "EventEmitter", (PyObject *)&EmitterType);
    Py_INCREF(&ScopeType);
    PyModule_AddObject(m, "StateScope", (PyObject *)&ScopeType);
    Py_INCREF(&FSMType);
    PyModule_AddObject(m, "FSM", (PyObject *)&FSMType);
    Py_INCREF(&SlotBaseType);
    PyModule_AddObject(m, "SlotBase", (PyObject *)&SlotBaseType);
    Py_INCREF(&CHType);
    PyModule_AddObject(m, "ClaimHandleBase", (PyObject *)&CHType);
    Py_INCREF(&NQueueType);
    PyModule_AddObject(m, "Queue", (PyObject *)&NQueueType);
    Py_INCREF(&QNodeType);
    PyModule_AddObject(m, "QueueNode", (PyObject *)&QNodeType);
    Py_INCREF(&CTType);
    PyModule_AddObject(m, "ClaimTicket", (PyObject *)&CTType);
    Py_INCREF(&SlotKitType);
    PyModule_AddObject(m, "SlotKit", (PyObject *)&SlotKitType);
    Py_INCREF(&SlotDispatchType);
    PyModule_AddObject(m, "SlotDispatch", (PyObject *)&SlotDispatchType);
    Py_INCREF(&CoDelType);
    PyModule_AddObject(m, "ControlledDelay", (PyObject *)&CoDelType);
    Py_INCREF(&LatHistType);
    PyModule_AddObject(m, "LatencyHistogram", (PyObject *)&LatHistType);
    Py_INCREF(&PoolLatType);
    PyModule_AddObject(m, "PoolLatency", (PyObject *)&PoolLatType);
    return m;
}
