"""HTTP(S) agents: pooled keep-alive HTTP clients (reference lib/agent.js).

``HttpAgent``/``HttpsAgent`` auto-create one ConnectionPool per host
(static or DNS-resolved via resolver_for_ip_or_domain), hand claimed
connections to requests, and run the optional HTTP ping health check on
idle connections.  The reference duck-types node's ``http.Agent``; the
rebuild keeps the same architecture against its own HttpRequest
machinery (cueball_amd.http_client):

- ``add_request(req, options)`` — the low-level socket-event protocol:
  claim -> req.on_socket(conn); 'free' => release, 'close' => disable
  leak check + release (benefit of the doubt), req 'abort' => cancel or
  close, 'agentRemove' => hold until close (lib/agent.js:275-396).
- ``request(...)``/``request_async(...)`` — convenience wrappers.
- the opt-in ``retry`` option routes ``request()``/``request_async()``
  through a retry driver (cueball_amd.retry): per-try and total
  timeouts, retries on another backend, a retry budget per host.
  ``add_request()`` with a caller-built request never retries.
- the opt-in ``hedge`` option sends a slow ``request()`` a second time,
  to another backend, and takes the first answer (cueball_amd.hedge);
  with ``retry`` also on, every try of the retry driver is hedged.
- ping checker: claims the exact idle socket and runs GET <ping>; a 5xx
  or error closes the connection, anything else releases it
  (lib/agent.js:398-455, PingAgent :530-569).
"""

from __future__ import annotations

import ssl as mod_ssl
from typing import Any, Callable, Dict, Mapping, Optional

from . import hedge as mod_hedge
from . import retry as mod_retry
from . import utils as mod_utils
from .connection import TcpConnection
from .errors import CueballError
from .events import EventEmitter
from .fsm import get_loop
from .http_client import HttpRequest, HttpResponse
from .logutil import CueballLogger, default_logger
from .pool import ConnectionPool
from .resolver import resolver_for_ip_or_domain

__all__ = ["Agent", "HttpAgent", "HttpsAgent", "FakeSocket", "PingAgent"]

#: TLS/connect fields passed through from request options to the socket
#: constructor (lib/agent.js:96-97)
PASS_FIELDS = ("ssl_context", "server_hostname", "cert", "key", "ca",
               "rejectUnauthorized")


class FakeSocket(EventEmitter):
    """Error-delivery stub: addRequest cannot return an async error any
    other way (lib/agent.js:306-317, :518-527)."""

    _is_fake_socket = True

    def read(self) -> None:
        return None

    def destroy(self) -> None:
        return None


class Agent(EventEmitter):
    # The retry option's state.  Class-level defaults, so that an agent
    # without the option carries no extra instance attribute.
    #: the validated ``retry`` option, defaults filled in
    cba_retry: Optional[Dict[str, Any]] = None
    #: the same as the driver reads it (retry.RetryPolicy)
    cba_retry_policy: Any = None
    #: host -> retry.RetryHost: budget, counters, pending backoffs
    cba_retry_hosts: Optional[Dict[str, Any]] = None
    _retry_metrics: Optional[tuple] = None
    # The hedge option's state, likewise.
    #: the validated ``hedge`` option, defaults filled in
    cba_hedge: Optional[Dict[str, Any]] = None
    #: the same as the driver reads it (hedge.HedgePolicy)
    cba_hedge_policy: Any = None
    #: host -> hedge.HedgeHost: budget, latency window, counters
    cba_hedge_hosts: Optional[Dict[str, Any]] = None
    _hedge_metrics: Optional[tuple] = None
    #: the validated ``claimBalancing`` option, likewise; a copy goes
    #: to every pool
    cba_balancing: Optional[Dict[str, Any]] = None
    #: the validated ``claimQueue`` option, likewise
    cba_queue: Optional[Dict[str, Any]] = None
    #: the validated ``claimAffinity`` option, likewise
    cba_affinity: Optional[Dict[str, Any]] = None
    #: the validated ``concurrencyLimit`` option, likewise: every pool
    #: gets a copy and keeps a limit of its own
    cba_limit: Optional[Dict[str, Any]] = None

    def __init__(self, options: Dict[str, Any]) -> None:
        super().__init__()
        if not isinstance(options.get("defaultPort"), int):
            raise TypeError("options.defaultPort is required")
        if not isinstance(options.get("protocol"), str):
            raise TypeError("options.protocol is required")

        self.collector = mod_utils.create_error_metrics(options)
        self._loop = get_loop(options.get("loop"))

        self.default_port: int = options["defaultPort"]
        self.protocol: str = options["protocol"] + ":"
        self.service = "_" + options["protocol"] + "._tcp"

        self.keep_alive = True
        self.tcp_ka_delay = options.get("tcpKeepAliveInitialDelay")

        self.pools: Dict[str, ConnectionPool] = {}
        self.pool_resolvers: Dict[str, Any] = {}
        self.pool_external_resolvers: Dict[str, Any] = {}
        self.resolvers = options.get("resolvers")
        log: CueballLogger = options.get("log") or default_logger()
        self.log = log.child(component="CueBallAgent")
        self.cba_stopped = False

        spares = options.get("spares")
        maximum = options.get("maximum")
        if not isinstance(spares, int) or not isinstance(maximum, int):
            raise TypeError("options.spares and options.maximum required")
        self.spares = spares
        self.maximum = maximum

        self.cba_ping: Optional[str] = options.get("ping")
        self.cba_ping_interval: Optional[float] = options.get("pingInterval")

        recovery = options.get("recovery")
        if not isinstance(recovery, dict):
            raise TypeError("options.recovery is required")
        mod_utils.assert_recovery(recovery.get("default"), "recovery.default")
        self.cba_recovery = recovery

        self.cba_err_on_empty = bool(options.get("errorOnEmpty"))
        self.cba_latency_stats = options.get("latencyStats")
        # handed to every pool and DNS resolver this agent creates
        srv_ranking = options.get("srvRanking")
        if srv_ranking is not None and not isinstance(srv_ranking, bool):
            raise TypeError("options.srvRanking must be a bool")
        self.cba_srv_ranking = bool(srv_ranking)
        # likewise handed to every pool; validated here so that a bad
        # value fails at construction, not at the first request
        self.cba_max_conn_age, self.cba_conn_age_spread = \
            mod_utils.assert_connection_age(options)
        # Likewise.  An agent closes leases on purpose (non-keep-alive
        # responses, aborts) and releases after the socket closed, so
        # by default neither counts against a backend: what does is a
        # socket error under a request and a failed ping.
        self.cba_outlier = mod_utils.assert_outlier_detection(
            options, count_default=False)

        # Request retries (opt-in): see the "retries" section below.
        # Off means not one attribute is set here.
        retry = mod_utils.assert_retry_policy(options)
        if retry is not None:
            self.cba_retry = retry
            self.cba_retry_policy = mod_retry.RetryPolicy(retry)
            self.cba_retry_hosts = {}
            self._register_retry_metrics()
        # Request hedging (opt-in), likewise: see "hedging" below.
        hedge = mod_utils.assert_hedge_policy(options)
        if hedge is not None:
            self.cba_hedge = hedge
            self.cba_hedge_policy = mod_hedge.HedgePolicy(hedge)
            self.cba_hedge_hosts = {}
            self._register_hedge_metrics()

        # Claim balancing (opt-in) is the pools' business; validated
        # here so that a bad value fails at construction.
        balancing = mod_utils.assert_claim_balancing(options)
        if balancing is not None:
            self.cba_balancing = balancing
        # The claim queue (opt-in), likewise.
        queue = mod_utils.assert_claim_queue(options)
        if queue is not None:
            self.cba_queue = queue
        # Key affinity (opt-in), likewise.
        affinity = mod_utils.assert_claim_affinity(options)
        if affinity is not None:
            self.cba_affinity = affinity
        # The concurrency limit (opt-in), likewise.
        limit = mod_utils.assert_concurrency_limit(options)
        if limit is not None:
            self.cba_limit = limit

        for host in options.get("initialDomains") or ():
            self._add_pool(host, {})

    # -- pool management --------------------------------------------------
    def _add_pool(self, host: str, options: Dict[str, Any]) -> None:
        if self.cba_stopped:
            raise CueballError("Cannot add a pool to a stopped agent")
        def_port = self.default_port
        port_opt = options.get("port")
        if isinstance(port_opt, str):
            port_opt = int(port_opt)
        if isinstance(port_opt, int):
            def_port = port_opt

        use_external = options.get("resolver") is not None
        if use_external:
            res = options["resolver"]
        else:
            resolver_config = {
                "resolvers": self.resolvers,
                "service": self.service,
                "defaultPort": def_port,
                "recovery": self.cba_recovery,
                "log": self.log,
                "loop": self._loop,
            }
            if self.cba_srv_ranking:
                resolver_config["srvRanking"] = True
            res = resolver_for_ip_or_domain({
                "input": host,
                "resolverConfig": resolver_config,
            })
            if isinstance(res, Exception):
                raise res

        tls = self.protocol == "https:"
        agent = self

        def construct_socket(backend: Dict[str, Any]) -> TcpConnection:
            sslctx = options.get("ssl_context")
            if tls and sslctx is None:
                sslctx = mod_ssl.create_default_context()
                if options.get("ca") is not None:
                    sslctx = mod_ssl.create_default_context(
                        cadata=options["ca"])
                if options.get("rejectUnauthorized") is False:
                    sslctx.check_hostname = False
                    sslctx.verify_mode = mod_ssl.CERT_NONE
            conn = TcpConnection(
                {
                    "key": backend.get("key"),
                    "name": backend.get("name") or host,
                    "address": backend.get("address") or backend.get("name"),
                    "port": backend.get("port") or def_port,
                },
                loop=agent._loop,
                tls=tls,
                ssl_context=sslctx,
                server_hostname=options.get("server_hostname")
                or backend.get("name") or host,
            )
            if agent.tcp_ka_delay is not None:
                def enable_ka() -> None:
                    sock = None
                    if conn._transport is not None:
                        sock = conn._transport.get_extra_info("socket")
                    if sock is not None:
                        import socket as mod_socket
                        sock.setsockopt(mod_socket.SOL_SOCKET,
                                        mod_socket.SO_KEEPALIVE, 1)
                        # node's setKeepAlive(initialDelay) also sets the
                        # idle time before the first probe; map the ms
                        # option onto TCP_KEEPIDLE (whole seconds, >=1).
                        idle_s = max(1, int(agent.tcp_ka_delay / 1000))
                        for opt in ("TCP_KEEPIDLE", "TCP_KEEPALIVE"):
                            if hasattr(mod_socket, opt):
                                try:
                                    sock.setsockopt(
                                        mod_socket.IPPROTO_TCP,
                                        getattr(mod_socket, opt), idle_s)
                                except OSError:
                                    pass
                                break
                conn.on("connect", enable_ka)
            return conn

        pool_opts: Dict[str, Any] = {
            "resolver": res,
            "domain": host,
            "constructor": construct_socket,
            "maximum": self.maximum,
            "spares": self.spares,
            "log": self.log,
            "recovery": self.cba_recovery,
            "collector": self.collector,
            "loop": self._loop,
        }
        if self.cba_latency_stats is not None:
            pool_opts["latencyStats"] = self.cba_latency_stats
        if self.cba_srv_ranking:
            pool_opts["srvRanking"] = True
        if self.cba_max_conn_age is not None:
            pool_opts["maxConnectionAge"] = self.cba_max_conn_age
            pool_opts["connectionAgeSpread"] = self.cba_conn_age_spread
        if self.cba_outlier is not None:
            pool_opts["outlierDetection"] = dict(self.cba_outlier)
        if self.cba_balancing is not None:
            pool_opts["claimBalancing"] = dict(self.cba_balancing)
        if self.cba_queue is not None:
            pool_opts["claimQueue"] = dict(self.cba_queue)
        if self.cba_affinity is not None:
            pool_opts["claimAffinity"] = {
                "loadFactor": self.cba_affinity["loadFactor"]}
        if self.cba_limit is not None:
            pool_opts["concurrencyLimit"] = dict(self.cba_limit)
        if self.cba_ping is not None:
            pool_opts["checkTimeout"] = self.cba_ping_interval or 30000
            pool_opts["checker"] = \
                lambda hdl, sock: self._check_socket(host, hdl, sock)

        self.log.debug("CueBallAgent creating new pool", host=host)
        self.pools[host] = ConnectionPool(pool_opts)
        if use_external:
            self.pool_external_resolvers[host] = res
        else:
            res.start()
            self.pool_resolvers[host] = res

    def get_pool(self, host: str) -> Optional[ConnectionPool]:
        return self.pools.get(host)

    def get_latency_stats(self) -> Dict[str, Any]:
        """Per-host ``ConnectionPool.get_latency_stats()``."""
        return {host: pool.get_latency_stats()
                for host, pool in self.pools.items()}

    def recycle(self, host: Optional[str] = None) -> int:
        """``ConnectionPool.recycle()`` on one host's pool, or on every
        pool when `host` is None; returns the total number of
        connections marked."""
        if host is not None:
            pool = self.pools.get(host)
            if pool is None:
                raise CueballError('No pool for host "%s"' % host)
            return pool.recycle()
        return sum(pool.recycle() for pool in self.pools.values())

    def get_outlier_stats(self) -> Dict[str, Any]:
        """Per-host ``ConnectionPool.get_outlier_stats()``."""
        return {host: pool.get_outlier_stats()
                for host, pool in self.pools.items()}

    def get_balancing_stats(self, host: str) -> Dict[str, Any]:
        """``ConnectionPool.get_balancing_stats()`` of `host`'s pool."""
        return self._pool_for(host).get_balancing_stats()

    def get_queue_stats(self, host: str) -> Dict[str, Any]:
        """``ConnectionPool.get_queue_stats()`` of `host`'s pool."""
        return self._pool_for(host).get_queue_stats()

    def get_affinity_stats(self, host: str) -> Dict[str, Any]:
        """``ConnectionPool.get_affinity_stats()`` of `host`'s pool."""
        return self._pool_for(host).get_affinity_stats()

    def get_limit_stats(self, host: str) -> Dict[str, Any]:
        """``ConnectionPool.get_limit_stats()`` of `host`'s pool."""
        return self._pool_for(host).get_limit_stats()

    def _pool_for(self, host: str) -> ConnectionPool:
        pool = self.pools.get(host)
        if pool is None:
            raise CueballError('No pool for host "%s"' % host)
        return pool

    def eject_backend(self, host: str, key: str,
                      ms: Optional[float] = None) -> bool:
        """``ConnectionPool.eject_backend(key, ms)`` on `host`'s pool."""
        return self._pool_for(host).eject_backend(key, ms)

    def reinstate_backend(self, host: str, key: str) -> bool:
        """``ConnectionPool.reinstate_backend(key)`` on `host`'s pool."""
        return self._pool_for(host).reinstate_backend(key)

    def create_pool(self, host: str,
                    options: Optional[Dict[str, Any]] = None) -> None:
        if host in self.pools:
            raise CueballError("Attempting to create a pool for a hostname "
                               "that already has one.")
        self._add_pool(host, dict(options or {}))

    def create_connection(self, options: Any = None,
                          connect_listener: Any = None) -> None:
        """UNIX-socket path: unsupported, as in the reference
        (lib/agent.js:492-495)."""
        raise CueballError("UNIX domain sockets not supported")

    def is_stopped(self) -> bool:
        return self.cba_stopped

    def stop(self, cb: Optional[Callable] = None) -> None:
        if self.cba_stopped:
            raise CueballError("Cannot stop a CueBallAgent that has "
                               "already stopped")
        self.cba_stopped = True
        self.log.debug("CueBallAgent stopping all pools")
        if self.cba_retry_hosts:
            # a request between two tries holds nothing a pool could
            # fail: end it here
            err = CueballError("CueBallAgent is stopped and cannot handle "
                               "new requests")
            for rhost in self.cba_retry_hosts.values():
                rhost.stop(err)
        if self.cba_hedge_hosts:
            # no second attempt is started on a stopped agent
            for hhost in self.cba_hedge_hosts.values():
                hhost.stop()
        hosts = list(self.pools.keys())
        remaining = {"n": len(hosts)}

        def done_one() -> None:
            remaining["n"] -= 1
            if remaining["n"] == 0 and cb is not None:
                self._loop.call_soon(lambda: cb(None))

        if not hosts:
            if cb is not None:
                self._loop.call_soon(lambda: cb(None))
            return

        for host in hosts:
            pool = self.pools.pop(host)
            res = self.pool_resolvers.pop(host, None)
            ext = res is None
            if ext:
                res = self.pool_external_resolvers.pop(host, None)

            def make_on_stopped(p=pool, r=res, is_ext=ext):
                fired = {"done": False}

                def on_state(st: str) -> None:
                    if fired["done"] or st != "stopped":
                        return
                    fired["done"] = True
                    if not is_ext and r is not None and \
                            not r.is_in_state("stopped"):
                        r.stop()
                    done_one()
                return on_state

            if pool.is_in_state("stopped"):
                if not ext and res is not None and \
                        not res.is_in_state("stopped"):
                    res.stop()
                done_one()
            else:
                pool.on("stateChanged", make_on_stopped())
                pool.stop()

    # -- the request path ---------------------------------------------------
    def add_request(self, req: HttpRequest,
                    options_or_host: Any, port: Optional[int] = None) -> None:
        """Low-level: claim a connection and wire the socket-event
        protocol (lib/agent.js:275-396)."""
        if self.cba_stopped:
            raise CueballError("CueBallAgent is stopped and cannot handle "
                               "new requests")
        if isinstance(options_or_host, str):
            options: Dict[str, Any] = {"host": options_or_host}
            if port is not None:
                options["port"] = port
        else:
            options = dict(options_or_host or {})
        host = options.get("host") or options.get("hostname")
        if not isinstance(host, str):
            raise TypeError("hostname is required")
        if host not in self.pools:
            self._add_pool(host, options)
        pool = self.pools[host]
        if isinstance(req, _TryRequest) and (
                self.cba_retry is not None or self.cba_hedge is not None
                or req.try_priority is not None
                or req.try_affinity is not None):
            _TryTicket(self, pool, req)
        else:
            _RequestTicket(self, pool, req)

    def request(self, options_or_host: Any, method: str = "GET",
                path: str = "/", headers: Optional[Dict[str, str]] = None,
                body: Optional[bytes] = None,
                cb: Optional[Callable] = None,
                retry: Any = None, hedge: Any = None,
                priority: Optional[int] = None,
                affinityKey: Any = None) -> Any:
        """Convenience: run one request; cb(err, response) after the
        body has fully arrived.

        On an agent with the ``retry`` option the request runs under
        the retry driver and a ``retry.RetriedRequest`` is returned;
        ``retry=False`` switches the driver off for this call, a
        mapping overrides keys of the agent's policy (all but
        ``budget``) for this call.

        On an agent with the ``hedge`` option the request, or each try
        of the retry driver, is a ``hedge.HedgedTry``, which is what is
        returned when only ``hedge`` is on; ``hedge=False`` switches
        hedging off for this call, a mapping overrides keys of the
        agent's policy (all but ``budget``, ``window`` and
        ``minSamples``).

        ``priority`` is the claim option of that name, for an agent
        with ``claimQueue``: the class of the claim of every try and of
        every hedge attempt of this request.

        ``affinityKey`` (bytes or str) is the claim option of that
        name, for an agent with ``claimAffinity``: every try and every
        hedge attempt of this request prefers the backends in the key's
        order.  A retry or a hedge attempt avoids the backends tried
        before it, and so lands on the key's next choice."""
        if isinstance(options_or_host, str):
            host = options_or_host
        else:
            host = options_or_host.get("host")
        if priority is not None:
            # checked here, against the agent's claimQueue, so that a
            # bad value fails at the call and not in some later try
            mod_utils.assert_claim_priority(priority, self.cba_queue,
                                            "priority=", "an agent")
        if affinityKey is not None:
            affinityKey = mod_utils.assert_affinity_key(
                affinityKey, self.cba_affinity, "affinityKey=", "an agent")
        if retry is not None or self.cba_retry is not None or \
                hedge is not None or self.cba_hedge is not None:
            policy = self._retry_policy_for(retry)
            hpolicy = self._hedge_policy_for(hedge)
            if policy is not None or hpolicy is not None:
                return self._request_driven(
                    policy, hpolicy, options_or_host, host, method, path,
                    headers, body, cb, priority, affinityKey)
        if priority is None and affinityKey is None:
            req = HttpRequest(method, path, headers=headers, body=body,
                              host=host)
        else:
            req = _TryRequest(method, path, headers=headers, body=body,
                              host=host)
            req.try_priority = priority
            req.try_affinity = affinityKey

        if cb is not None:
            def on_resp(resp: HttpResponse) -> None:
                if resp.complete:
                    cb(None, resp)
                else:
                    resp.on("end", lambda: cb(None, resp))

            req.on("response", on_resp)
            req.on("error", lambda e: cb(e, None))
        self.add_request(req, options_or_host)
        return req

    async def request_async(self, options_or_host: Any, method: str = "GET",
                            path: str = "/",
                            headers: Optional[Dict[str, str]] = None,
                            body: Optional[bytes] = None,
                            retry: Any = None,
                            hedge: Any = None,
                            priority: Optional[int] = None,
                            affinityKey: Any = None) -> HttpResponse:
        fut = self._loop.create_future()

        def cb(err: Optional[BaseException],
               resp: Optional[HttpResponse]) -> None:
            if fut.done():
                return
            if err is not None:
                fut.set_exception(err)
            else:
                fut.set_result(resp)

        if retry is None and hedge is None and priority is None and \
                affinityKey is None:
            self.request(options_or_host, method, path, headers, body, cb)
        else:
            self.request(options_or_host, method, path, headers, body, cb,
                         retry=retry, hedge=hedge, priority=priority,
                         affinityKey=affinityKey)
        return await fut

    # -- retries --------------------------------------------------------------
    #
    # With the ``retry`` option, request() hands the request to a
    # retry.RetriedRequest.  Each try is a fresh HttpRequest that goes
    # through add_request() like any other; it is a _TryRequest, so
    # that its ticket (_TryTicket) can pass the backends to avoid to the
    # claim and note which backend the try was served by.

    _RETRY_METRICS = (
        ("cueball_agent_retries_total",
         "Requests retried by the agent, by host and reason"),
        ("cueball_agent_retry_budget_exhausted_total",
         "Retries the agent's retry budget denied, by host"),
        ("cueball_agent_request_timeouts_total",
         "Per-try and total request timeouts that fired, by host"),
    )

    def _register_retry_metrics(self) -> None:
        try:
            self._retry_metrics = tuple(
                self.collector.counter(name=name, help=help_)
                for name, help_ in self._RETRY_METRICS)
        except (AttributeError, ValueError, TypeError):
            self._retry_metrics = None  # foreign collector

    def _retry_counted(self, host: str, counter: str) -> None:
        metrics = self._retry_metrics
        if metrics is None:
            return
        if counter == "retry-budget-exhausted":
            metrics[1].increment({"host": host})
        elif counter.startswith("retry-"):
            metrics[0].increment({"host": host, "reason": counter[6:]})
        elif counter.startswith("timeout-"):
            metrics[2].increment({"host": host, "kind": counter[8:]})

    def _retry_policy_for(self, retry: Any) -> Any:
        """The policy of one call, None for a call without the driver."""
        if retry is None:
            return self.cba_retry_policy
        if retry is False:
            return None
        if self.cba_retry is None:
            if isinstance(retry, Mapping):
                raise ValueError("retry= needs an agent that was created "
                                 "with options.retry")
            raise TypeError("retry= must be False or a mapping")
        return mod_retry.RetryPolicy(
            mod_utils.override_retry_policy(self.cba_retry, retry))

    def _request_driven(self, policy: Any, hpolicy: Any,
                        options_or_host: Any,
                        host: Any, method: str, path: str,
                        headers: Optional[Dict[str, str]],
                        body: Optional[bytes],
                        cb: Optional[Callable],
                        priority: Optional[int] = None,
                        affinity: Optional[bytes] = None) -> Any:
        """One request under the retry driver (`policy`), the hedge
        driver (`hpolicy`), or both: then every try of the retry driver
        is a hedged one.  Both drivers start a try or an attempt through
        start_real_try below, so that is where `priority` and
        `affinity` (the bytes of ``affinityKey=``) reach every claim of
        the request."""
        if not isinstance(host, str):
            if isinstance(options_or_host, Mapping):
                host = options_or_host.get("hostname")
            if not isinstance(host, str):
                raise TypeError("hostname is required")

        def start_real_try(avoid: tuple) -> HttpRequest:
            req = _TryRequest(method, path, headers=headers, body=body,
                              host=host)
            if avoid:
                req.try_avoid = avoid
            if priority is not None:
                req.try_priority = priority
            if affinity is not None:
                req.try_affinity = affinity
            self.add_request(req, options_or_host)
            return req

        if hpolicy is not None:
            hhost = self.cba_hedge_hosts.get(host)
            if hhost is None:
                hhost = self.cba_hedge_hosts[host] = mod_hedge.HedgeHost(
                    host, self.cba_hedge_policy, self._loop.time,
                    self._hedge_counted, self._hedge_delay_changed)
                if self.cba_hedge_policy.delay is not None:
                    self._hedge_delay_changed(
                        host, self.cba_hedge_policy.delay)

            def has_idle(avoid: tuple) -> bool:
                pool = self.pools.get(host)
                return pool is not None and pool.has_idle_connection(avoid)

            def hedged_try(avoid: tuple) -> Any:
                return mod_hedge.HedgedTry(
                    self._loop, hpolicy, hhost, method, start_real_try,
                    avoid, has_idle, self.is_stopped)

        if policy is None:
            rreq = hedged_try(())
        else:
            rhost = self.cba_retry_hosts.get(host)
            if rhost is None:
                rhost = self.cba_retry_hosts[host] = mod_retry.RetryHost(
                    host, self.cba_retry["budget"], self._retry_counted)
            start_try = start_real_try if hpolicy is None else \
                (lambda avoid: hedged_try(avoid).start())
            rreq = mod_retry.RetriedRequest(self._loop, policy, rhost,
                                            method, start_try,
                                            self.is_stopped)
        if cb is not None:
            def on_resp(resp: HttpResponse) -> None:
                if resp.complete:
                    cb(None, resp)
                else:
                    resp.on("end", lambda: cb(None, resp))

            rreq.on("response", on_resp)
            rreq.on("error", lambda e: cb(e, None))
        return rreq.start()

    def get_retry_stats(self) -> Dict[str, Any]:
        """Per host that has seen a request: ``{"active", "retrying",
        "limit", "counters": {...}}``; ``limit`` is None without a
        budget.  Empty on an agent without ``retry``."""
        return {host: rhost.stats()
                for host, rhost in (self.cba_retry_hosts or {}).items()}

    # -- hedging ----------------------------------------------------------------
    #
    # With the ``hedge`` option, request() hands the request (or, under
    # the retry driver, each of its tries) to a hedge.HedgedTry.  Its
    # one or two attempts are _TryRequests like the tries of a retried
    # request, so that the second one's claim can avoid the backend of
    # the first.

    def _register_hedge_metrics(self) -> None:
        try:
            self._hedge_metrics = (
                self.collector.counter(
                    name="cueball_agent_hedges_total",
                    help="Hedged requests of the agent, by host and "
                         "outcome"),
                self.collector.gauge(
                    name="cueball_agent_hedge_delay_seconds",
                    help="The delay after which a request is hedged, "
                         "by host"))
        except (AttributeError, ValueError, TypeError):
            self._hedge_metrics = None  # foreign collector

    def _hedge_counted(self, host: str, counter: str) -> None:
        metrics = self._hedge_metrics
        if metrics is not None:
            # "hedge-sent" -> outcome "sent"
            metrics[0].increment({"host": host, "outcome": counter[6:]})

    def _hedge_delay_changed(self, host: str, ms: float) -> None:
        metrics = self._hedge_metrics
        if metrics is not None:
            metrics[1].set(ms / 1000.0, {"host": host})

    def _hedge_policy_for(self, hedge: Any) -> Any:
        """The hedge policy of one call, None for a call without
        hedging."""
        if hedge is None:
            return self.cba_hedge_policy
        if hedge is False:
            return None
        if self.cba_hedge is None:
            if isinstance(hedge, Mapping):
                raise ValueError("hedge= needs an agent that was created "
                                 "with options.hedge")
            raise TypeError("hedge= must be False or a mapping")
        return mod_hedge.HedgePolicy(
            mod_utils.override_hedge_policy(self.cba_hedge, hedge))

    def get_hedge_stats(self) -> Dict[str, Any]:
        """Per host that has seen a request under the driver: ``{"active",
        "hedging", "limit", "delayMs", "samples", "latency",
        "counters": {...}}``; ``delayMs`` is None while the adaptive
        estimate has too few samples.  Empty on an agent without
        ``hedge``."""
        return {host: hhost.stats()
                for host, hhost in (self.cba_hedge_hosts or {}).items()}

    # -- health checking -----------------------------------------------------
    def _check_socket(self, host: str, handle: Any, socket: Any) -> None:
        t1 = self._loop.time()
        log = self.log.child(component="CueBallAgentPing", domain=host,
                             path=self.cba_ping)
        agent = PingAgent({"protocol": self.protocol, "socket": socket,
                           "log": log})
        req = HttpRequest("GET", self.cba_ping, host=host)

        def on_resp(resp: HttpResponse) -> None:
            def finish() -> None:
                if 500 <= resp.status_code < 600:
                    log.warn("got a 5xx code, closing",
                             statusCode=resp.status_code,
                             latency=round(
                                 (self._loop.time() - t1) * 1000, 2))
                    handle.close()
                else:
                    log.debug("health check ok, releasing",
                              statusCode=resp.status_code)
                    handle.release()

            if resp.complete:
                finish()
            else:
                resp.on("end", finish)

        req.on("response", on_resp)
        req.once("error", lambda e: (
            log.warn("check failed: %s", e,
                     latency=round((self._loop.time() - t1) * 1000, 2)),
            handle.close()))
        agent.add_request(req, {})


class _RequestTicket:
    """One request's claim + socket-event protocol (the closure-free
    form of lib/agent.js:296-396; this sits on the HTTP hot path)."""

    __slots__ = ("agent", "req", "waiter", "conn", "sock")

    def __init__(self, agent: "Agent", pool: Any, req: HttpRequest) -> None:
        self.agent = agent
        self.req = req
        self.conn: Any = None
        self.sock: Any = None
        req.once("abort", self.on_abort)
        self.waiter = pool.claim(
            {"errorOnEmpty": agent.cba_err_on_empty}, self.claimed)

    def claimed(self, err: Optional[BaseException], connh: Any = None,
                socket: Any = None) -> None:
        self.waiter = None
        if err is not None:
            fakesock = FakeSocket()
            self.req.on_socket(fakesock)
            self.agent._loop.call_soon(
                lambda: fakesock.emit("error", err))
            return
        self.conn = connh
        self.sock = socket
        socket.once("free", self.on_free)
        socket.once("close", self.on_close)
        socket.once("agentRemove", self.on_agent_remove)
        self.req.on_socket(socket)

    def on_abort(self) -> None:
        if self.waiter is not None:
            self.waiter.cancel()
            self.waiter = None
        if self.conn is not None:
            sock = self.sock
            sock.remove_listener("close", self.on_close)
            sock.remove_listener("free", self.on_free)
            sock.remove_listener("agentRemove", self.on_agent_remove)
            self.conn.close()
            self.conn = None
            self.sock = None

    def on_close(self) -> None:
        sock = self.sock
        sock.remove_listener("free", self.on_free)
        sock.remove_listener("agentRemove", self.on_agent_remove)
        self.req.remove_listener("abort", self.on_abort)
        # A 'close' straight after a normally-completed request is
        # indistinguishable from a premature close; give it the benefit
        # of the doubt: disable the leak check and release rather than
        # close (lib/agent.js:328-360).
        conn = self.conn
        conn.disable_release_leak_check()
        conn.release()
        self.conn = None
        self.sock = None

    def on_free(self) -> None:
        sock = self.sock
        sock.remove_listener("close", self.on_close)
        sock.remove_listener("agentRemove", self.on_agent_remove)
        self.req.remove_listener("abort", self.on_abort)
        self.conn.release()
        self.conn = None
        self.sock = None

    def on_agent_remove(self) -> None:
        # Upgrade etc.: the socket now belongs to someone else; hold
        # the lease until 'close'.
        self.sock.remove_listener("free", self.on_free)
        self.req.remove_listener("abort", self.on_abort)


class _TryRequest(HttpRequest):
    """One try of a retried request, or one attempt of a hedged try
    (see Agent._request_driven)."""

    #: backend keys the try's claim is to avoid
    try_avoid: tuple = ()
    #: the class of the try's claim (``priority=``), None for the
    #: pool's default
    try_priority: Optional[int] = None
    #: the affinity key of the try's claim (``affinityKey=``), as bytes
    try_affinity: Optional[bytes] = None
    #: the try's claim handle and its slot, None until claimed
    try_handle: Any = None
    try_slot: Any = None

    @property
    def try_backend(self) -> Optional[str]:
        """The key of the backend the try was claimed on, None until
        then.  Looked up only when a try has failed."""
        slot = self.try_slot
        return None if slot is None else slot.get_backend().get("key")


class _TryTicket(_RequestTicket):
    """A _TryRequest's ticket: the claim avoids the backends the
    request has failed on, and the try learns where it landed."""

    __slots__ = ()

    def __init__(self, agent: "Agent", pool: Any, req: _TryRequest) -> None:
        self.agent = agent
        self.req = req
        self.conn = None
        self.sock = None
        req.once("abort", self.on_abort)
        options: Dict[str, Any] = {"errorOnEmpty": agent.cba_err_on_empty}
        if req.try_avoid:
            options["avoidBackends"] = req.try_avoid
        if req.try_priority is not None:
            options["priority"] = req.try_priority
        if req.try_affinity is not None:
            options["affinityKey"] = req.try_affinity
        self.waiter = pool.claim(options, self.claimed)

    def claimed(self, err: Optional[BaseException], connh: Any = None,
                socket: Any = None) -> None:
        if err is None:
            req = self.req
            req.try_handle = connh
            req.try_slot = connh.ch_slot
        _RequestTicket.claimed(self, err, connh, socket)


class PingAgent(EventEmitter):
    """Runs a request on one specific, already-claimed socket
    (lib/agent.js:530-569)."""

    def __init__(self, options: Dict[str, Any]) -> None:
        super().__init__()
        self.protocol = options["protocol"]
        self.keep_alive = True
        self.pa_socket = options["socket"]
        self.log = options.get("log")

    def add_request(self, req: HttpRequest,
                    options: Optional[Dict[str, Any]] = None) -> None:
        sock = self.pa_socket

        def on_abort() -> None:
            sock.remove_listener("free", on_free)
            sock.remove_listener("agentRemove", on_agent_remove)

        def on_free() -> None:
            sock.remove_listener("agentRemove", on_agent_remove)
            req.remove_listener("abort", on_abort)

        def on_agent_remove() -> None:
            sock.remove_listener("free", on_free)
            req.remove_listener("abort", on_abort)

        sock.once("free", on_free)
        sock.once("agentRemove", on_agent_remove)
        req.once("abort", on_abort)
        req.on_socket(sock)


class HttpAgent(Agent):
    def __init__(self, options: Dict[str, Any]) -> None:
        options = dict(options)
        options["protocol"] = "http"
        options.setdefault("defaultPort", 80)
        super().__init__(options)


class HttpsAgent(Agent):
    def __init__(self, options: Dict[str, Any]) -> None:
        options = dict(options)
        options["protocol"] = "https"
        options.setdefault("defaultPort", 443)
        super().__init__(options)
