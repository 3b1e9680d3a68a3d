"""Shared fixtures of the claim-queue tests: a pool of one backend with
two connections, both claimed, so that every further claim has to wait;
labelled claims whose outcomes are logged in the order they happen."""

from cueball_amd.testing import settle

from balance_kit import Kit


class QueueKit(Kit):
    """``cq`` is the ``claimQueue`` option, None for a pool without it.
    ``log`` holds ``(label, outcome)`` in callback order: outcome is
    "served" or the error's class name; ``errors`` maps labels to the
    error objects."""

    def __init__(self, loop, cq=None, **opts):
        if cq is not None:
            opts["claimQueue"] = cq
        opts.setdefault("backends", ("b1",))
        opts.setdefault("per", 2)
        super().__init__(loop, **opts)
        self.log = []
        self.errors = {}
        self.boxes = {}
        self.holders = []

    async def busy(self):
        """Claim every connection; afterwards each claim queues."""
        self.holders = [self.claim() for _ in range(len(self.conns))]
        await settle(self.loop)
        for box in self.holders:
            assert box.get("err", 1) is None, box
        assert self.pool.get_stats()["idleConnections"] == 0
        return self

    def queue(self, label, priority=None, **options):
        """One labelled claim; does not settle."""
        if priority is not None:
            options["priority"] = priority
        box = {"label": label, "fired": 0}

        def cb(err, hdl=None, conn=None):
            box["fired"] += 1
            box.update(err=err, hdl=hdl, conn=conn)
            if err is None:
                self.log.append((label, "served"))
            else:
                self.log.append((label, type(err).__name__))
                self.errors[label] = err

        box["waiter"] = self.pool.claim(options, cb)
        box["waiter"].test_label = label
        self.boxes[label] = box
        return box

    async def queue_all(self, spec):
        """``spec``: an iterable of labels or (label, priority) pairs,
        queued one loop turn apart."""
        for item in spec:
            if isinstance(item, tuple):
                self.queue(*item)
            else:
                self.queue(item)
            await settle(self.loop)

    def order(self):
        """Labels of the waiters, head first."""
        out = []
        self.pool.p_waiters.for_each(
            lambda hdl, node: out.append(hdl.test_label))
        return out

    async def serve_all(self):
        """Release the holders, then every claim that is served, one at
        a time, until nothing waits; returns the labels in the order
        they were served."""
        start = len(self.log)
        for box in self.holders:
            box["hdl"].release()
        self.holders = []
        await settle(self.loop)
        done = set()
        progressed = True
        while progressed:
            progressed = False
            for label, outcome in list(self.log[start:]):
                if outcome == "served" and label not in done:
                    done.add(label)
                    self.boxes[label]["hdl"].release()
                    await settle(self.loop)
                    progressed = True
        return [l for l, o in self.log[start:] if o == "served"]

    def served(self):
        return [l for l, o in self.log if o == "served"]

    def queue_stats(self):
        st = self.pool.get_queue_stats()
        assert sum(st["queued"]) == self.pool.get_stats()["waiterCount"]
        return st
