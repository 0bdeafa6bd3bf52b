"""PolicyCache: the reference cache's policy half over the device-resident policy table.

AutoUpdatingCache keeps the TASPolicy objects under "policies/<namespace>/<name>"
(telemetry-aware-scheduling/pkg/cache/autoupdating.go, cache/types.go:11-22) and
TelemetryPolicyController keeps them current (controller/controller.go:61-176): onAdd, onUpdate
and onDelete write the policy, register its strategies with the MetricEnforcer
(strategies/core/enforcer.go:64-103) and register each rule's metric with the metric cache.
Here the same decisions are made on the host, as TasCache makes the metric half's: every
policy gets a stable id, its row of the table installed by pas_tas_policies_set, and the verbs
by policy id (pas_tas_eval_policies, pas_tas_filter_requests_policies, the
pas_tas[_gas]_topk_policies* entry points) read that row where the reference reads the object
with cache.ReadPolicy.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .context import RULE_DTYPE, make_rules, parse_operator

SCHEDULEONMETRIC = "scheduleonmetric"
DESCHEDULE = "deschedule"
DONTSCHEDULE = "dontschedule"
STRATEGY_TYPES = (SCHEDULEONMETRIC, DESCHEDULE, DONTSCHEDULE)  # castStrategy (:94-108)

Rule = Tuple[str, str, int]  # (metric name, operator, target): TASPolicyRule


class TasPolicy(NamedTuple):
    """A TASPolicy object as the informer hands it over.  strategies: {strategy type: spec} in
    the order the controller is to walk them (the reference ranges over a Go map); a spec is
    the rule list [(metric, operator, target)], or {"policyName": .., "rules": [..]} when the
    object's own TASPolicyStrategy.PolicyName field is set."""
    namespace: str
    name: str
    strategies: Mapping[str, object]


def strategy_of(spec) -> Tuple[str, List[Rule]]:
    """(PolicyName, Rules) of a strategy spec; the zero value for a missing one (None)."""
    if spec is None:
        return "", []
    if isinstance(spec, Mapping):
        return str(spec.get("policyName") or ""), list(spec.get("rules") or [])
    return "", list(spec)


def strategy_equals(a: Tuple[str, Sequence[Rule]], b: Tuple[str, Sequence[Rule]]) -> bool:
    """deschedule.Strategy.Equals (deschedule/strategy.go:60-78): the same policy name and the
    same non-empty rule list (metric, target, operator per position)."""
    (na, ra), (nb, rb) = a, b
    if na != nb or not ra or len(ra) != len(rb):
        return False
    return all(x[0] == y[0] and int(x[2]) == int(y[2]) and x[1] == y[1] for x, y in zip(ra, rb))


def op_code(op: str) -> int:
    """pas_op of a TASPolicyRule operator; an unknown one becomes an invalid code, which the
    library skips where the rule is never evaluated and answers PAS_EINVAL where the
    reference's EvaluateRule would panic (operator.go:25)."""
    code = parse_operator(op)
    return code if code >= 0 else 3


class PolicyCache:
    """The policy half of the reference's cache and the controller that feeds it, over a
    context's resident policy table.  Single-threaded, as TasCache.

    `ctx` holds a TAS snapshot.  `metrics` is the metric half (a TasCache, or anything with
    write_metric(name), delete_metric(name) and metric_index): every rule of a registered
    strategy registers its metric there and unregisters it with the strategy.  Without one
    (`metrics=None`, a snapshot that nothing refreshes) `metric_names` gives the columns.

    The reference's calls, with their quirks as they are:
      write_policy / read_policy / delete_policy   WritePolicy, ReadPolicy, DeletePolicy, keyed
          by (namespace, name); read_policy raises KeyError where ReadPolicy returns its error.
      on_add(pol)      onAdd (:61-91): the policy is written, then for each strategy type of
          the policy: an invalid type ends the event there (the `return` at :76-79; the policy
          stays written and the strategies walked so far stay registered); the strategy gets
          the object's name (SetPolicyName drops the namespace), goes to the enforcer, and
          each of its rules registers its metric.
      on_update(old, new)   onUpdate (:111-149): the new policy is written over the old one,
          then ONLY the new policy's strategy types are walked.  For each, the old policy's
          strategy of that type (the zero value when the old policy has none) is removed from
          the enforcer by Equals -- with the old object's own PolicyName field, which nothing
          set to the object's name here, so a strategy registered by on_add under the object's
          name is found only when the field says the same -- and the old strategy's rules
          unregister their metrics; then the new strategy is added as in on_add.  A strategy
          type only the old policy has is neither removed nor are its metrics unregistered.
      on_delete(pol)   onDelete (:152-176): each strategy is removed by Equals under the
          object's name and its rules unregister their metrics; an invalid type ends the event
          before the policy is deleted.
    The enforcer registry is kept for the deschedule type, the only registered type that is
    Enforceable (core/enforcer.go:97-102): add drops a strategy Equals to a registered one,
    remove drops every registered strategy Equals to the one given.  `strategies` lists the
    registry as [(policy name, rules)] in registration order, which is what DescheduleEnforcer
    takes.  (Cleanup's label removal on RemoveStrategy is not part of this class.)

    Ids and the table.  A policy keeps the id it got when first written until delete_policy;
    a freed id is reused by the next new policy and its row is empty meanwhile.  Row i holds
    the policy's dontschedule rules and its scheduleonmetric Rules[0], metric names resolved to
    the snapshot's columns as MetricsExtender resolves them (a name without a column: -1).
    Every event ends with one pas_tas_policies_set; snapshot_changed (MetricsExtender's hook)
    resolves the names again and sets the table again after the snapshot's columns changed.
    """

    def __init__(self, ctx, metrics=None, metric_names: Optional[Sequence[Optional[str]]] = None):
        self.ctx = ctx
        self.metrics = metrics
        self._metric_index: Dict[str, int] = {
            m: i for i, m in enumerate(metric_names or []) if m is not None}
        self.policies: Dict[Tuple[str, str], TasPolicy] = {}
        self.ids: Dict[Tuple[str, str], int] = {}
        self._rows: List[Optional[Tuple[str, str]]] = []  # id -> key, None for a free id
        self.strategies: List[Tuple[str, List[Rule]]] = []  # the deschedule registry
        self._prio = make_rules([], [], [])
        self._set_table()

    # ------------------------------------------------------------ the cache's policy calls
    def write_policy(self, namespace: str, name: str, policy: TasPolicy):
        key = (namespace, name)
        self.policies[key] = policy
        if key not in self.ids:
            free = [i for i, k in enumerate(self._rows) if k is None]
            if free:
                self._rows[free[0]] = key
                self.ids[key] = free[0]
            else:
                self.ids[key] = len(self._rows)
                self._rows.append(key)

    def read_policy(self, namespace: str, name: str) -> TasPolicy:
        return self.policies[(namespace, name)]

    def delete_policy(self, namespace: str, name: str):
        key = (namespace, name)
        if key in self.policies:
            del self.policies[key]
            self._rows[self.ids.pop(key)] = None
            while self._rows and self._rows[-1] is None:  # the table ends at the last id held
                self._rows.pop()

    # ------------------------------------------------------------ what the verbs ask
    def get(self, key: Tuple[str, str]) -> Optional[Dict[str, List[Rule]]]:
        """The policy as MetricsExtender's dict holds one: {strategy type: rules}; None for a
        policy the cache does not hold."""
        pol = self.policies.get(key)
        if pol is None:
            return None
        return {t: strategy_of(spec)[1] for t, spec in pol.strategies.items()}

    def id_of(self, key: Tuple[str, str]) -> int:
        """The policy's row of the table (KeyError for a policy the cache does not hold)."""
        return self.ids[key]

    def ids_of(self, keys: Sequence[Tuple[str, str]]) -> np.ndarray:
        """The rows of a pod batch's policies as int32 [len(keys)], -1 for a policy the cache
        does not hold: the pod_policy array of the verbs and top-k entry points by policy id,
        which read -1 as no dontschedule rules and no prio rule."""
        return np.fromiter((self.ids.get(key, -1) for key in keys), dtype=np.int32,
                           count=len(keys))

    def prio_of(self, policy_id: int):
        """The host pas_rule of row policy_id's scheduleonmetric rule; metric -1: none."""
        return self._prio[policy_id]

    @property
    def metric_index(self) -> Dict[str, int]:
        return self.metrics.metric_index if self.metrics is not None else self._metric_index

    # ------------------------------------------------------------ the controller's events
    def on_add(self, pol: TasPolicy):
        self.write_policy(pol.namespace, pol.name, pol)
        for stype, spec in pol.strategies.items():
            if stype not in STRATEGY_TYPES:
                break
            _, rules = strategy_of(spec)
            self._add_strategy(stype, (pol.name, rules))
            for rule in rules:
                self._write_metric(rule[0])
        self._set_table()

    def on_update(self, old: TasPolicy, new: TasPolicy):
        self.write_policy(new.namespace, new.name, new)
        for stype, spec in new.strategies.items():
            if stype not in STRATEGY_TYPES:
                break
            old_strategy = strategy_of(old.strategies.get(stype))  # (its own PolicyName field)
            self._remove_strategy(stype, old_strategy)
            for rule in old_strategy[1]:
                self._delete_metric(rule[0])
            _, rules = strategy_of(spec)
            self._add_strategy(stype, (new.name, rules))
            for rule in rules:
                self._write_metric(rule[0])
        self._set_table()

    def on_delete(self, pol: TasPolicy):
        for stype, spec in pol.strategies.items():
            if stype not in STRATEGY_TYPES:
                self._set_table()
                return
            _, rules = strategy_of(spec)
            self._remove_strategy(stype, (pol.name, rules))
            for rule in rules:
                self._delete_metric(rule[0])
        self.delete_policy(pol.namespace, pol.name)
        self._set_table()

    def snapshot_changed(self, gen=None, node_names=None,
                         metric_names: Optional[Sequence[Optional[str]]] = None):
        """The snapshot's columns changed (a set, a reshape): the rules' metric names are
        resolved again and the table is set again.  The arguments are MetricsExtender's; only
        metric_names is read, and only by a cache without a metric half."""
        if self.metrics is None and metric_names is not None:
            self._metric_index = {m: i for i, m in enumerate(metric_names) if m is not None}
        self._set_table()

    # ------------------------------------------------------------ host side
    def _add_strategy(self, stype: str, strategy):
        if stype != DESCHEDULE:  # not Enforceable: AddStrategy stores nothing
            return
        if not any(strategy_equals(s, strategy) for s in self.strategies):
            self.strategies.append((strategy[0], list(strategy[1])))

    def _remove_strategy(self, stype: str, strategy):
        if stype != DESCHEDULE:
            return
        self.strategies[:] = [s for s in self.strategies if not strategy_equals(s, strategy)]

    def _write_metric(self, name: str):
        if self.metrics is not None:
            self.metrics.write_metric(name)

    def _delete_metric(self, name: str):
        if self.metrics is not None:
            self.metrics.delete_metric(name)

    def table(self):
        """(rules, rule_off, prio) as pas_tas_policies_set takes them, from the policies held
        and the current columns."""
        index = self.metric_index
        metric, op, target, off = [], [], [], [0]
        pm, po, pt = [], [], []
        for key in self._rows:
            strategies = self.get(key) if key is not None else {}
            for m, o, t in strategies.get(DONTSCHEDULE) or []:
                metric.append(index.get(m, -1))  # not cached: skipped (strategy.go:28-32)
                op.append(op_code(o))
                target.append(int(t))
            off.append(len(metric))
            # getSchedulingRule (telemetryscheduler.go:115-124): the first rule, with a metric
            # name; ReadMetric's error (:130-133) is the empty list as well
            prio = strategies.get(SCHEDULEONMETRIC) or []
            if prio and prio[0][0] and prio[0][0] in index:
                pm.append(index[prio[0][0]])
                po.append(op_code(prio[0][1]))
                pt.append(int(prio[0][2]))
            else:
                pm.append(-1), po.append(0), pt.append(0)
        return make_rules(metric, op, target), np.array(off, np.int32), make_rules(pm, po, pt)

    def _set_table(self):
        rules, off, prio = self.table()
        self.ctx.tas_policies_set(rules, off, prio)
        self._prio = np.ascontiguousarray(prio, dtype=RULE_DTYPE)
